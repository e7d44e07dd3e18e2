"""CPU: the host side of the validation transforms on the device (ucd_val_image_path / ucd_val_label_path, csrc/datapipe.hip) -
the symbols, Resize + CenterCrop as numbers against Pillow's own resized size, the refusals that are heard before any device call,
and the switch."""
import pytest
import torch

from ucd_amd import datapipe, hip, switches

PIL = pytest.importorskip("PIL.Image")

# source (H0, W0), S -> resized (oh, ow), window (i, j)
CASES = [((37, 50), 33, (33, 44), (0, 6)),          # (44 - 33) / 2 = 5.5 -> 6: the half goes to the even neighbour, up
         ((37, 48), 33, (33, 42), (0, 4)),          # (42 - 33) / 2 = 4.5 -> 4: down
         ((50, 37), 33, (44, 33), (6, 0)),
         ((20, 31), 33, (33, 51), (0, 9)),
         ((131, 200), 33, (33, 50), (0, 8)),
         ((33, 33), 33, (33, 33), (0, 0)),
         ((33, 70), 33, (33, 70), (0, 18)),
         ((16, 160), 33, (33, 330), (0, 148)),
         ((375, 500), 64, (64, 85), (0, 10)),
         ((375, 500), 513, (513, 684), (0, 86))]


def test_symbols_are_declared_and_resolve():
    assert "ucd_val_image_path" in hip.SIGNATURES and "ucd_val_label_path" in hip.SIGNATURES
    lib = hip.load()
    assert lib.ucd_val_image_path is not None and lib.ucd_val_label_path is not None
    assert lib.ucd_version() == 100


@pytest.mark.parametrize("src,S,resized,window", CASES)
def test_resize_center_crop_params(src, S, resized, window):
    H0, W0 = src
    oh, ow, i, j = datapipe.resize_center_crop_params(H0, W0, S)
    assert (oh, ow) == resized and (i, j) == window
    # transform.Resize(S) hands (oh, ow) to Pillow: the size of what comes back; CenterCrop's arithmetic by hand
    short, long_ = min(H0, W0), max(H0, W0)
    other = int(S * long_ / short)
    pi = PIL.new("L", (W0, H0)).resize((S, other) if W0 <= H0 else (other, S), PIL.NEAREST)
    assert pi.size == (ow, oh) and min(oh, ow) == S
    assert (i, j) == (int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0)))
    assert 0 <= i <= oh - S and 0 <= j <= ow - S


def test_both_half_way_cases_are_in_the_table():
    halves = {(r[1] - S) / 2.0: w[1] for _, S, r, w in CASES if (r[1] - S) % 2}
    assert halves[5.5] == 6 and halves[4.5] == 4


def test_cpu_tensors_are_refused():
    img, lab = torch.zeros(37, 50, 3, dtype=torch.uint8), torch.zeros(37, 50, dtype=torch.uint8)
    p = [datapipe.resize_center_crop_params(37, 50, 33)]
    with pytest.raises(RuntimeError, match="GPU only"):
        datapipe.DeviceValImagePath()([img], p, (33, 33))
    with pytest.raises(RuntimeError, match="GPU only"):
        datapipe.DeviceValLabelPath(torch.arange(256, dtype=torch.uint8))([lab], p, (33, 33))


@pytest.mark.parametrize("params,out_hw", [((33, 44, 0, 12), (33, 33)),        # 12 + 33 > 44
                                           ((33, 44, -1, 6), (33, 33)),
                                           ((33, 44, 1, 6), (33, 33)),         # 1 + 33 > 33
                                           ((37, 50, 0, 0), (38, 50)),         # full size, one row too many
                                           ((33, 44, 0, 6), (0, 33))])
def test_a_window_outside_the_resized_extent_is_refused(params, out_hw):
    img, lab = torch.zeros(37, 50, 3, dtype=torch.uint8), torch.zeros(37, 50, dtype=torch.uint8)
    with pytest.raises(ValueError):
        datapipe.DeviceValImagePath()([img], [params], out_hw)
    with pytest.raises(ValueError):
        datapipe.DeviceValLabelPath(torch.arange(256, dtype=torch.uint8))([lab], [params], out_hw)


def test_wrong_dtype_or_shape_is_refused():
    p = [(33, 44, 0, 6)]
    images = datapipe.DeviceValImagePath()
    for bad in (torch.zeros(37, 50, 3), torch.zeros(37, 50, dtype=torch.uint8), torch.zeros(37, 50, 4, dtype=torch.uint8),
                torch.zeros(3, 37, 50, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            images([bad], p, (33, 33))
    labels = datapipe.DeviceValLabelPath(torch.arange(256, dtype=torch.uint8))
    for bad in (torch.zeros(37, 50, dtype=torch.int64), torch.zeros(37, 50, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            labels([bad], p, (33, 33))
    with pytest.raises(ValueError):
        images([], [], (33, 33))


def test_the_library_refuses_bad_arguments_before_any_launch():
    lib = hip.load()
    one = 1                                                      # any non-null address: nothing is read before the checks
    assert lib.ucd_val_image_path(None, one, 1, 33, 33, 3, 37, 0, 0, 0, 0, 1, 1, 1, one, one, one, None) != 0
    assert b"ucd_val_image_path" in lib.ucd_last_error()
    for B, oh, ow, kmax, hmax, mode in ((0, 33, 33, 3, 37, 0), (1, 0, 33, 3, 37, 0), (1, 33, -1, 3, 37, 0), (1, 33, 33, 2, 37, 0),
                                        (1, 33, 33, 3, 0, 0), (1, 33, 33, 3, 37, 2), (1, 70000, 33, 3, 37, 0)):
        assert lib.ucd_val_image_path(one, one, B, oh, ow, kmax, hmax, mode, 0, 0, 0, 1, 1, 1, one, one, one, None) != 0
    assert lib.ucd_val_label_path(one, one, 1, 33, 33, None, one, one, None) != 0
    assert b"ucd_val_label_path" in lib.ucd_last_error()
    for B, oh, ow in ((0, 33, 33), (1, 0, 33), (1, 33, 0), (1, 70000, 33)):
        assert lib.ucd_val_label_path(one, one, B, oh, ow, one, one, one, None) != 0


def test_switch_defaults_to_the_device_path():
    assert switches.DEFAULTS["UCD_VAL_DEVICE"] == "1"
    assert "UCD_VAL_DEVICE" in switches.snapshot()
