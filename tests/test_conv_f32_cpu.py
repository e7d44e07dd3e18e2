"""CPU: the fp32 split-bf16 convolution kernels (csrc/conv_f32.hip) - exported symbols, the opt-in switch and the routing gate
of ucd_amd/blocks.py as a function of layer shapes (no GPU)."""
import torch

from ucd_amd import blocks, hip, switches


def test_library_exports_the_f32_conv_entry_points():
    lib = hip.load()
    for name in ("ucd_conv_f32", "ucd_conv_f32_wgrad", "ucd_conv_f32_wgrad_workspace_bytes"):
        assert name in hip.SIGNATURES
        assert getattr(lib, name) is not None


def test_switch_defaults_off():
    assert switches.DEFAULTS["UCD_F32_OWN_CONV"] == "0"


def test_workspace_bytes_follow_the_shape_contract():
    lib = hip.load()
    assert lib.ucd_conv_f32_wgrad_workspace_bytes(26136, 256, 1024, 1) % (256 * 1024 * 4) == 0
    assert lib.ucd_conv_f32_wgrad_workspace_bytes(26136, 256, 2048, 9) % (256 * 9 * 2048 * 4) == 0
    for bad in ((1000, 48, 64, 1), (1000, 64, 48, 1), (1000, 64, 64, 3), (0, 64, 64, 1)):
        assert lib.ucd_conv_f32_wgrad_workspace_bytes(*bad) == 0


def test_entry_points_refuse_shapes_off_the_grid():
    """Each call below is valid but for the one argument named in its comment and must be refused before any launch.  Where a GPU
    is present the operands are real device buffers that cover every extent the calls declare, so even a regressed host check
    could not make a kernel touch memory outside them; without one the (aligned) addresses are never dereferenced."""
    lib = hip.load()
    elems = 65536 * 66 + 64
    if torch.cuda.is_available():
        bufs = [torch.zeros(elems, dtype=torch.float32, device="cuda") for _ in range(3)]
        a, w, y = (t.data_ptr() for t in bufs)
    else:
        a, w, y = 1 << 20, 1 << 28, 1 << 29
    assert lib.ucd_conv_f32(a, 48, w, 48, y, 64, 1000, 64, 48, 1, 0, 0, 0, 0, None) == -1           # K off the grid
    assert lib.ucd_conv_f32(a, 64, w, 64, y, 48, 1000, 48, 64, 1, 0, 0, 0, 0, None) == -1           # N off the grid
    assert lib.ucd_conv_f32(a + 4, 64, w, 64, y, 64, 1000, 64, 64, 1, 0, 0, 0, 0, None) == -1       # unaligned base
    assert lib.ucd_conv_f32(a, 66, w, 64, y, 64, 1000, 64, 64, 1, 0, 0, 0, 0, None) == -1           # unaligned pitch
    assert lib.ucd_conv_f32(a, 64, w, 576, y, 64, 1001, 64, 64, 9, 10, 10, 1, 0, None) == -1        # M not whole 10 x 10 maps
    assert lib.ucd_conv_f32(a, 64, w, 64, y, 64, 1000, 64, 64, 9, 10, 10, 1, 0, None) == -1         # pitch of w below 9 K
    assert lib.ucd_conv_f32_wgrad(a, 64, w, 48, 1000, 64, 48, 1, 0, 0, 0, y, None, 0, None) == -1   # K off the grid
    assert lib.ucd_conv_f32_wgrad(a, 64, w, 64, 1001, 64, 64, 9, 10, 10, 1, y, None, 0, None) == -1  # M not whole maps
    assert lib.ucd_conv_f32_wgrad(a, 64, w, 64, 65536, 64, 64, 1, 0, 0, 0, y, None, 0, None) == -1  # workspace missing


def test_routing_gate_as_a_function_of_shapes():
    g = blocks._own_f32_conv
    # the network's stride-1 layers at B = 24, 513^2 (and the 2 x 513^2 test batch)
    for M in (24 * 129 * 129, 24 * 65 * 65, 24 * 33 * 33, 2 * 33 * 33):
        for K, N in ((64, 256), (256, 64), (256, 1024), (1024, 256), (2048, 512), (512, 2048), (2048, 256), (1024, 256)):
            assert g(M, K, N, 1)
            assert blocks._own_f32_wgrad(M, K, N, 1) == (min(K, N) >= 128)
        for K, N in ((64, 64), (128, 128), (256, 256), (512, 512), (2048, 256)):
            assert g(M, K, N, 9)
            assert blocks._own_f32_wgrad(M, K, N, 9) == (min(K, N) >= 128)
        assert not g(M, 64, 64, 1)                 # measured slower than MIOpen fp32 (129^2: 51.5 vs 43.7 us)
    assert not g(24, 2048, 256, 1)                 # image-pooling branch on a 1 x 1 map
    assert not g(26136, 256, 21, 1)                # classifier head
    assert not g(26136, 3, 64, 1)
    assert not g(26136, 48, 64, 1) and not g(26136, 64, 48, 9)
    assert not g(26136, 64, 64, 49)                # 7 x 7


def _conv(cls, cin, cout, **kw):
    return cls(cin, cout, **kw) if cls is blocks.Conv1x1 else cls(cin, cout, 3, **kw)


def test_layer_gate_needs_the_switch_fp32_gpu_and_stride_one():
    c1 = blocks.Conv1x1(256, 64)
    c3 = blocks.Conv3x3(256, 256, 3, stride=1, padding=2, dilation=2, bias=False)
    x = torch.zeros(2, 256, 33, 33)
    switches.set("UCD_F32_OWN_CONV", "1")
    try:
        # CPU tensors never take the kernels
        assert not blocks._f32_conv_ok(c1, x) and not blocks._f32_conv_ok(c3, x)
        # strided, stem-like and biased layers stay on the library whatever the device
        strided = blocks.Conv2d(256, 256, 3, stride=2, padding=1, bias=False)
        stem = blocks.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        head = blocks.Conv2d(256, 64, 1, bias=True)
        for conv in (strided, stem, head):
            assert not blocks._f32_conv_ok(conv, x)
    finally:
        switches.unset("UCD_F32_OWN_CONV")
    assert not blocks._f32_conv_ok(c1, x)
