"""CPU: the host half of the contrastive-loss launch (ucd_pixcon_loss_plan, csrc/pixcon_loss*.hip).  The plan names the
kernels that serve a call (fp32 with the anchor block's probability rows in LDS, fp32 "wide" with those rows read from global
memory, fp16 planned, fp16 fixed-split), the split counts and the dynamic LDS of both sweeps; ucd_pixcon_loss launches with
exactly these numbers.  Nothing here needs a device.

The LDS expressions below restate the launch code of the commit BEFORE the plan existed (pixcon_loss.hip: lds1 / lds2 of the fp32
launch; pixcon_loss_f16.hip: lds1n / lds2 of the fixed-split launch; pixcon_loss_f16p.hip: lds_base / lds_prob of the planned
launch), so that K <= 110 (fp32) and K <= 112 (fp16) provably keep the launch they had."""
import ctypes as C

import pytest

from ucd_amd import hip

F32, F16, F16_SPLIT = 0, 1, 2
PATH_F32, PATH_F32_WIDE, PATH_F16_PLANNED, PATH_F16_SPLIT = 1, 2, 3, 4
EINVAL, EUNSUPPORTED = -1, -4
LDS_LIMIT = 160 * 1024
SIZES = (128, 3072, 26136)          # one anchor block; the ADE per-rank shape 3 x 32 x 32; the full VOC shape 24 x 33 x 33

# constants of the kernels as the earlier launch code used them
TJ, BI, N, PITCH32, PITCH16, RING, MAX_SPLIT = 32, 128, 256, 256 + 4, 256 + 24, 4, 16


def plan(BHW, K, prec, use_prob=1, T=0.07):
    """dict of the plan's answers, or (error code, message)."""
    lib = hip.load()
    path, chunk, n1, n2 = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    l1, l2, ws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = lib.ucd_pixcon_loss_plan(BHW, K, prec, use_prob, T, C.addressof(path), C.addressof(chunk), C.addressof(n1),
                                  C.addressof(n2), C.addressof(l1), C.addressof(l2), C.addressof(ws))
    if rc:
        return rc, lib.ucd_last_error().decode()
    return dict(path=path.value, chunk=chunk.value, n1=n1.value, n2=n2.value, lds1=l1.value, lds2=l2.value, ws=ws.value)


def parent_split(BHW):
    ns = -(-1024 // -(-BHW // BI))
    return max(1, min(ns, MAX_SPLIT))


def parent_lds_f32(K, use_prob):
    lds1 = (2 * TJ * PITCH32 + 2 * TJ) * 4
    KP2 = ((K + 1) & ~1) if use_prob else 0
    return lds1, lds1 + (2 * TJ + BI) * (KP2 + 1) * 4


def parent_lds_f16_split(K, use_prob):
    KP16 = (K + 15) // 16 * 16 if use_prob else 0
    lds1n = 3 * TJ * PITCH16 * 2 + 3 * (TJ + 4) * 4
    return lds1n, 3 * TJ * PITCH16 * 2 + 3 * TJ * 4 + 3 * TJ * (2 * KP16 + 8) * 2


def parent_lds_f16_planned(K, use_prob):
    KP16 = (K + 15) // 16 * 16 if use_prob else 0
    base = RING * TJ * PITCH16 * 2 + RING * 8 * 4 + 16
    return base, (base + RING * TJ * (2 * KP16 + 8) * 2) if use_prob else base


def parent_planned_eligible(BHW, K, use_prob, T):
    return 1.4426950408889634 / T <= 24.0 and -(-BHW // BI) < 1024 and (not use_prob or K <= 32)


@pytest.mark.parametrize("prec", [F32, F16, F16_SPLIT])
def test_every_k_is_planned_within_the_lds_and_the_workspace(prec):
    """K = 1 .. 255, use_prob 0 / 1, three sizes: the plan succeeds, both sweeps ask for at most 160 KiB, the split counts are the
    ones the launch always used, and ucd_pixcon_loss_workspace_bytes covers what the plan lays out."""
    lib = hip.load()
    for BHW in SIZES:
        for use_prob in (0, 1):
            for K in range(1, 256):
                p = plan(BHW, K, prec, use_prob)
                assert isinstance(p, dict), (BHW, K, use_prob, p)
                assert 0 < p["lds1"] <= LDS_LIMIT and 0 < p["lds2"] <= LDS_LIMIT, (BHW, K, use_prob, p)
                assert lib.ucd_pixcon_loss_workspace_bytes(BHW, N, K) >= p["ws"] > 0, (BHW, K, p)
                assert p["chunk"] == 0 or 0 < p["chunk"] < K, (K, p)
                if p["path"] == PATH_F16_PLANNED:
                    assert (p["n1"], p["n2"]) == (0, 0)
                else:
                    assert p["n1"] == p["n2"] == parent_split(BHW), (BHW, p)


def test_few_class_calls_keep_the_launch_they_had():
    """fp32 K <= 110 and fp16 K <= 112: no class chunk, the path and the LDS bytes of the launch code before the plan."""
    for BHW in SIZES:
        for use_prob in (0, 1):
            for K in range(1, 113):
                if K <= 110:
                    p = plan(BHW, K, F32, use_prob)
                    assert (p["path"], p["chunk"]) == (PATH_F32, 0), (K, p)
                    assert (p["lds1"], p["lds2"]) == parent_lds_f32(K, use_prob), (K, use_prob, p)
                p = plan(BHW, K, F16_SPLIT, use_prob)
                assert (p["path"], p["chunk"]) == (PATH_F16_SPLIT, 0), (K, p)
                assert (p["lds1"], p["lds2"]) == parent_lds_f16_split(K, use_prob), (K, use_prob, p)
                for T in (0.07, 0.05):
                    p = plan(BHW, K, F16, use_prob, T)
                    if parent_planned_eligible(BHW, K, use_prob, T):
                        assert (p["path"], p["chunk"]) == (PATH_F16_PLANNED, 0), (K, T, p)
                        assert (p["lds1"], p["lds2"]) == parent_lds_f16_planned(K, use_prob), (K, use_prob, p)
                    else:
                        assert (p["path"], p["chunk"]) == (PATH_F16_SPLIT, 0), (K, T, p)
                        assert (p["lds1"], p["lds2"]) == parent_lds_f16_split(K, use_prob), (K, use_prob, p)


def test_many_class_paths_and_their_lds():
    """Past the old bounds: fp32 moves the anchor block's probability rows out of the LDS (two contrast tiles' rows of K rounded to
    even, + 1 float of pitch, remain), fp16 keeps its one formula.  The figures are DESIGN.md's table."""
    base32 = (2 * TJ * PITCH32 + 2 * TJ) * 4
    for K, want32, want16 in ((111, base32 + 2 * TJ * 113 * 4, 110976 - 192 * 64), (141, base32 + 2 * TJ * 143 * 4, 110976),
                             (255, 132608, 153984)):
        p = plan(3072, K, F32)
        assert (p["path"], p["chunk"], p["lds1"], p["lds2"]) == (PATH_F32_WIDE, 0, base32, want32), (K, p)
        for prec in (F16, F16_SPLIT):
            p = plan(3072, K, prec)
            assert (p["path"], p["chunk"], p["lds2"]) == (PATH_F16_SPLIT, 0, want16), (K, p)
    assert plan(3072, 255, F32, use_prob=0)["path"] == PATH_F32          # without the probabilities K plays no part
    # 1024 anchor blocks or more: the planned form does not apply
    assert plan(1024 * 128, 16, F16)["path"] == PATH_F16_SPLIT and plan(1023 * 128, 16, F16)["path"] == PATH_F16_PLANNED


@pytest.mark.parametrize("prec", [F32, F16, F16_SPLIT])
def test_class_bounds_are_refused_with_the_documented_codes(prec):
    got = plan(3072, 0, prec)
    assert got[0] == EINVAL and "1 <= K <= 255" in got[1], got
    got = plan(3072, 256, prec)
    assert got[0] == EUNSUPPORTED and "1 <= K <= 255" in got[1], got
    assert plan(3072, 256, prec, use_prob=0)[0] == EUNSUPPORTED
    assert plan(3072, -1, prec, use_prob=0)[0] == EINVAL
    assert isinstance(plan(3072, 0, prec, use_prob=0), dict)             # ucd_pixcon_loss_given_p: no probabilities, K = 0
    assert plan(0, 16, prec)[0] == EINVAL and plan(3072, 16, prec, T=0.0)[0] == EINVAL
    assert plan(3072, 16, 3)[0] == EINVAL


def test_python_binding():
    p = hip.pixcon_loss_plan(3072, 141, "f32")
    assert p["path"] == "f32/wide" and p["class_chunk"] == 0 and p["lds_sweep2"] <= LDS_LIMIT
    assert hip.pixcon_loss_plan(3072, 16, "f16")["path"] == "f16/planned"
    assert hip.pixcon_loss_plan(3072, 141, "f16")["path"] == "f16/split"
    assert hip.pixcon_loss_plan(3072, 101, "f32", use_prob=True, temperature=0.07)["path"] == "f32"
    with pytest.raises(RuntimeError, match="1 <= K <= 255"):
        hip.pixcon_loss_plan(3072, 256, "f32")
