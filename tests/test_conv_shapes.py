"""The launch shape of the fp32 convs (conv_shape, csrc/kernels_conv.hip; kd_conv_launch_shape) against the choices the
launcher made before that function existed: tests/golden/conv_launch_shapes.json, recorded from that launcher's own code
by tests/golden/make_conv_launch_shapes.py (tests/golden/README.md), whose build_cases() is the table.  Host code only:
runs without a GPU."""
import ctypes as C
import importlib.util
import json
from pathlib import Path

import pytest

import helpers as H

GOLDEN_DIR = Path(__file__).parent / "golden"
GOLDEN = json.loads((GOLDEN_DIR / "conv_launch_shapes.json").read_text())
FIELDS = GOLDEN["shape_fields"]
SHAPES = [dict(zip(FIELDS, s)) for s in GOLDEN["shapes"]]


def _recipe():
    spec = importlib.util.spec_from_file_location("make_conv_launch_shapes", GOLDEN_DIR / "make_conv_launch_shapes.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECIPE = _recipe()
CASES = RECIPE.build_cases()   # (group, geometry, has, al16, cus), in the order of the recording


@pytest.fixture(scope="module")
def lib():
    return H.engine().load()


def query(lib, row):
    n = len(RECIPE.GEOM)
    geom, out = (C.c_int * n)(*row[:n]), (C.c_int * len(FIELDS))()
    has, al16, cus = row[n:]
    rc = lib.kd_conv_launch_shape(C.addressof(geom), has, al16, cus, C.addressof(out))
    return rc, dict(zip(FIELDS, out))


def test_table_is_the_recorded_one():
    """The table still is what the golden was recorded over, and holds every row test_kernels_gpu.test_conv_igemm runs."""
    assert RECIPE.cases_digest(CASES) == GOLDEN["cases_sha256"] and len(CASES) == len(SHAPES)
    rows = [SHAPES[i] for i, c in enumerate(CASES) if c[0] == "conv_igemm"]
    assert len(rows) == len(RECIPE.conv_igemm_rows())
    assert len({(s["igemm"], s["bm"], s["bn"]) for s in rows}) == 8   # between them they launch every variant


def test_golden_holds_every_choice():
    """What the recording had to contain, so that equality below pins every branch of the chooser."""
    assert {(s["igemm"], s["bm"], s["bn"]) for s in SHAPES} == {(0, 256, 128), (0, 128, 128), (0, 128, 64), (0, 64, 128),
                                                                (1, 128, 32), (1, 128, 64), (1, 64, 128), (1, 128, 128)}
    assert {s["ksplit"] > 1 for s in SHAPES} == {True, False} and min(s["ksplit"] for s in SHAPES) == 1
    assert {s["wide"] for s in SHAPES} == {0, 1}
    assert {s["seg_chunks"] > 0 for s in SHAPES} == {True, False}
    assert {cus for grp, _, _, _, cus in CASES if grp == "grid"} == {256, 120}   # the grid at two CU counts
    assert {g["wz_count"] for _, g, _, _, _ in CASES if g["wz_rows"]} == {16, 36}
    for bit in (1, 2, 4, 8, 16):   # every alignment flag occurs set and cleared on a pointer that is there
        assert {bool(al & bit) for _, _, has, al, _ in CASES if has & bit} == {True, False}


def test_conv_launch_shape_equals_the_recorded_choice(lib):
    wrong = []
    for case, want in zip(CASES, SHAPES):
        rc, got = query(lib, RECIPE.case_row(case))
        if rc or got != want:
            wrong.append((case, want, rc, got))
    assert not wrong, (len(wrong), wrong[:3])


def test_conv_launch_shape_refuses_a_batched_gemm_off_the_fast_path(lib):
    g = RECIPE.geom(1, 1, 256, 36, 64, wz_rows=128, wz_count=2)   # Cin % 32 != 0
    rc, _ = query(lib, RECIPE.case_row(("", g, 1, 1, 256)))
    assert rc != 0
