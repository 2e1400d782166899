"""CPU-side checks of the wide bucket ranges (up to 8 hits per line; include/rrl.h rrl_loss_forward_wide): the ABI, the
host-side argument validation, the range classification of rrl_hip.ops, and the checker (the CPU oracle) against the
reference's own values at wide ranges (tests/golden/loss_wide.npz, tests/golden/make_golden_wide.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, merge_by_point

@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def test_wide_symbols_exported_and_enum_matches_view_table(lib):
    from rrl_hip import ops
    header = open(os.path.join(ROOT, "include", "rrl.h")).read()
    table = header[header.index("#define RRL_WW_TABLE(X)"):header.index("#define RRL_WW_ENUM_")]
    names = re.findall(r"\bX\(([A-Z0-9]+),", table)
    assert len(names) == 16 and [n.upper() for n in ops._WW.index] == names  # the library-derived view table, in order
    offs = (ctypes.c_size_t * len(names))()
    assert lib.rrl_wide_workspace_layout(8, 4096, 4096, 10000, offs) == 0
    total = lib.rrl_wide_workspace_bytes(8, 4096, 4096, 10000)
    o = [int(v) for v in offs]
    assert o[0] == 0 and o == sorted(o) and all(v % 256 == 0 for v in o) and o[-1] < total
    # every field holds its view (the view table's sizes fit between the C offsets)
    dims = (8, 4096, 4096, 10000, 8)
    for i, name in enumerate(ops._WW.index):
        off, nbytes, dtype, shape = ops._WW.spec(dims, name)
        assert off == o[i] and nbytes == int(np.prod(shape)) * dtype.itemsize > 0
        assert o[i] + nbytes <= (o[i + 1] if i + 1 < len(o) else total)


def test_wide_entries_validate_on_the_host(lib):
    """Range and pointer errors are reported before any HIP call (no GPU needed); the narrow entries keep refusing."""
    fake = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    fw = lib.rrl_loss_forward_wide
    args = lambda s_m, e_m: (fake, fake, fake, fake, 1 << 40, fake, 1 << 40, fake, 1, 16, 16, 32, s_m, 1, e_m, 9, 0, 3, 0,  # noqa: E731
                             None, None)
    assert fw(*args(1, 10)) == -2 and fw(*args(0, 9)) == -2
    a = list(args(1, 9)); a[15] = 10  # e_n = 10
    assert fw(*a) == -2
    assert fw(None, fake, fake, fake, 1 << 40, fake, 1 << 40, fake, 1, 16, 16, 32, 1, 1, 9, 9, 0, 3, 0, None, None) == -1
    assert fw(fake, fake, fake, fake, 1 << 40, None, 1 << 40, fake, 1, 16, 16, 32, 1, 1, 9, 9, 0, 3, 0, None, None) == -1
    assert fw(fake, fake, fake, fake, 0, fake, 1 << 40, fake, 1, 16, 16, 32, 1, 1, 9, 9, 0, 3, 0, None, None) == -3
    assert lib.rrl_loss_backward_wide(None, 0, None, None, None, 1, 1, 1, 1, 0, None) == -1
    assert lib.rrl_loss_backward_wide(fake, 0, fake, fake, None, 1, 16, 16, 32, 0, None) == -3
    # the narrow entries are unchanged: a wide range is RRL_E_RANGE there
    assert lib.rrl_loss_reduce(fake, 1 << 40, fake, 1, 1, 1, 1, 1, 1, 9, 9, 0, None) == -2


def test_range_classification():
    from rrl_hip import ops
    assert ops._classify_range((1, 1, 5, 5)) == ((1, 1, 5, 5), False)
    assert ops._classify_range((2, 3, 4, 5)) == ((2, 3, 4, 5), False)
    for r in ((1, 1, 9, 9), (2, 3, 8, 9), (1, 1, 7, 5), (5, 5, 9, 9), (1, 1, 6, 2)):
        assert ops._classify_range(r) == (r, True) and ops._is_wide(r)
    for r in ((0, 1, 5, 5), (1, 0, 9, 9), (1, 1, 10, 9), (1, 1, 9, 10)):
        with pytest.raises(ValueError, match="1..8"):
            ops._classify_range(r)
        assert not ops._is_wide(r)
    assert ops._check_range((1, 1, 5, 5), "registration_loss") == (1, 1, 5, 5)
    with pytest.raises(ValueError, match=r"registration_loss .*ops\.intersection_loss"):
        ops._check_range((1, 1, 9, 9), "registration_loss")


W = load_golden("loss_wide.npz")
FIXTURES = [str(x) for x in W["fixtures"]]
RANGES = [tuple(int(v) for v in r) for r in W["ranges"]]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_at_wide_ranges(oracle, name):
    """The checker's pin at every stored wide range: loss <= 1e-6 relative, median to a few ulps, per-point gradient sums <= 1e-5."""
    g = load_golden(f"loss_{name}.npz")
    for i, rng in enumerate(RANGES):
        ref = oracle.loss(g["tri1"], g["tri2"], g["lines"], rng, want_D=True)
        if bool(W[f"{name}_r{i}_empty"]):
            assert ref["loss"] is None, (name, rng)
            continue
        want = float(W[f"{name}_r{i}_loss"])
        assert abs(float(ref["loss"]) - want) <= 1e-6 * abs(want), (name, rng, ref["loss"], want)
        # the median and the D values to a few ulps: the reference sums the squared differences in torch's own order, and on
        # ref_real1 at (1, 1, 9, 9) the median is such a value
        med, want_med = np.float32(ref["median"]), np.float32(W[f"{name}_r{i}_median"])
        assert abs(med - want_med) <= 4 * np.spacing(want_med), (name, rng, med, want_med)
        np.testing.assert_allclose(np.sort(ref["D"]), np.sort(W[f"{name}_r{i}_D"]), rtol=4e-6, atol=0)
        mine, theirs = merge_by_point(g["tri1"], ref["grad1"]), merge_by_point(g["tri1"], W[f"{name}_r{i}_grad1"])
        assert np.abs(mine - theirs).max() <= 1e-5 * np.abs(theirs).max() + 1e-9, (name, rng)


def test_oracle_grad2_matches_reference(oracle):
    name, rng = str(W["grad2_pair"]), tuple(int(v) for v in W["grad2_range"])
    g = load_golden(f"loss_{name}.npz")
    ref = oracle.loss(g["tri1"], g["tri2"], g["lines"], rng, want_grad2=True)
    assert abs(float(ref["loss"]) - float(W["grad2_loss"])) <= 1e-6 * abs(float(W["grad2_loss"]))
    for tri, mine, theirs in ((g["tri1"], ref["grad1"], W["grad2_grad1"]), (g["tri2"], ref["grad2"], W["grad2_grad2"])):
        a, b = merge_by_point(tri, mine), merge_by_point(tri, theirs)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-9
