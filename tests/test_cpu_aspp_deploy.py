"""Host logic of the ASPP_ResNet deployment path, no device needed: the ctypes mirror of ubr_aspp_front_desc against the
header, the stacked tile descriptors / keep windows of the whole-view segmenter, and load_model's `arch` argument."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from ubresnet_amd import _lib as L
from ubresnet_amd import deploy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "ubresnet_hip.h")

_FIELDS = ["dtype", "N", "H", "W", "C", "pad_", "x", "w", "bias", "y"]


def test_aspp_front_desc_layout_matches_header(tmp_path):
    D = L.AsppFrontDesc
    # int32 x6, ubr_tensor, two pointers, ubr_tensor
    assert C.sizeof(D) == 24 + 32 + 8 + 8 + 32
    assert [f[0] for f in D._fields_] == _FIELDS
    assert [getattr(D, f).offset for f in _FIELDS] == [0, 4, 8, 12, 16, 20, 24, 56, 64, 72]
    # the header declares the same members in the same order
    body = re.search(r"typedef struct \{([^}]*)\} ubr_aspp_front_desc;", open(HDR).read()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == _FIELDS, names
    assert "ubr_aspp_front" in L.SYMBOLS
    gcc = shutil.which("gcc")
    if gcc is not None:          # and a C compiler lays the struct out as ctypes does
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) { printf("%%zu", sizeof(ubr_aspp_front_desc));\n'
                       % HDR + "".join('printf(" %%zu", offsetof(ubr_aspp_front_desc, %s));\n' % f for f in _FIELDS) + "return 0; }\n")
        exe = tmp_path / "layout"
        r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
        assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in _FIELDS]


def test_library_exports_aspp_front():
    assert hasattr(L.lib(), "ubr_aspp_front")


@pytest.mark.parametrize("rows,cols,th,tw,ntiles", [(1008, 3456, 512, 832, 10), (100, 200, 64, 96, 6), (64, 96, 64, 96, 1)])
def test_stacked_tiles_and_keep_windows(rows, cols, th, tw, ntiles):
    P = 3
    tiles = deploy.view_tiles(rows, cols, P, th, tw, stacked=True)
    assert len(tiles) == ntiles and all(t[0] == 0 for t in tiles)
    # per-plane tiling of the same view: the same positions and keep windows, once per plane
    per_plane = deploy.view_tiles(rows, cols, P, th, tw, stacked=False)
    assert per_plane == [(p,) + t[1:] for p in range(P) for t in tiles]
    # keep windows partition the view
    cover = torch.zeros((rows, cols), dtype=torch.int32)
    for (_, r0, c0, kr0, kr1, kc0, kc1) in tiles:
        assert 0 <= kr0 < kr1 <= th and 0 <= kc0 < kc1 <= tw
        cover[r0 + kr0:min(r0 + kr1, rows), c0 + kc0:min(c0 + kc1, cols)] += 1
    assert int(cover.min()) == 1 and int(cover.max()) == 1
    # a stacked tile = `planes` consecutive single-plane crops at one origin (the crop kernel then writes [n, planes, th, tw])
    crop = deploy.stacked_crop_desc(tiles, P)
    assert len(crop) == P * ntiles
    for i, t in enumerate(tiles):
        for p in range(P):
            assert crop[P * i + p] == (p,) + t[1:]


class _Stub:
    """stands in for a model on a machine without a device: the segmenter's constructor reads these two attributes only"""

    def __init__(self, cin, ncls=3):
        self.conv1 = torch.nn.Conv2d(cin, 16, 7)
        self.conv11 = torch.nn.Conv2d(16, ncls, 7)


def test_segmenter_modes_without_a_device():
    seg = deploy.WholeViewSegmenter(_Stub(3), 1008, 3456, planes=3, batch=10)
    assert seg.stacked and seg.tiles_per_event == 10 and seg.cin == 3
    seg = deploy.WholeViewSegmenter(_Stub(1, 4), 1008, 3456, planes=3, batch=10)
    assert not seg.stacked and seg.tiles_per_event == 30 and seg.cin == 1
    with pytest.raises(ValueError):
        deploy.WholeViewSegmenter(_Stub(2), 1008, 3456, planes=3, batch=10)
    with pytest.raises(ValueError):          # 22 stacked tiles = 66 single-plane crop descriptors > UBR_MAX_TILES
        deploy.WholeViewSegmenter(_Stub(3), 1008, 3456, planes=3, batch=22)
    deploy.WholeViewSegmenter(_Stub(3), 1008, 3456, planes=3, batch=21)
    deploy.WholeViewSegmenter(_Stub(1), 1008, 3456, planes=3, batch=64)


def test_load_model_arch():
    from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
    from ubresnet_amd.models.ub_uresnet import UResNet
    m = deploy.load_model(None, "cpu", num_classes=3, input_channels=3, arch="aspp")
    assert isinstance(m, ASPP_ResNet) and not m.training and m.conv1.in_channels == 3 and m.conv11.out_channels == 3
    assert isinstance(deploy.load_model(None, "cpu", num_classes=4), UResNet)
    with pytest.raises(ValueError):
        deploy.load_model(None, "cpu", arch="resnet")
