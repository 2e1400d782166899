"""The host twin of the ball-query grouping (tests/group_refs.py) against the reference's own run
(tests/golden/ball_query_rpm.npz, recorded from rpm/models/pointnet_util.py query_ball_point and sample_and_group_multi by
make_golden_ball_query.py) and against a plain Python loop; the new entry in the header and the binding; and every refusal
that needs no GPU -- the Python layer's and the C entry's (fake pointers: nothing is launched)."""
import numpy as np
import pytest
import torch

import group_refs as GR
from conftest import load_golden

FAKE = 0x1000  # a non-NULL, aligned pointer that is never dereferenced
E_ARG = -1
BORDER_MAX = 0.01  # borderline rows: at most 1 % of a case's rows


@pytest.fixture(scope="module")
def golden():
    return load_golden("ball_query_rpm.npz")


def settings_of(golden, name):
    return [(float(r), int(k)) for r, k in golden[f"{name}_settings"]]


def tag(radius, nsample):
    return f"r{int(round(radius * 100)):03d}_k{nsample}"


def test_twin_indices_equal_the_reference_run(golden):
    """Every row without a borderline pair holds the recorded indices, in both forms of the pad rule; borderline rows are at
    most 1 % of a case's rows; truncation at nsample is covered."""
    names = [str(c) for c in golden["cases"]]
    assert len(names) == 5
    truncated = 0.0
    for name in names:
        x = golden[f"{name}_xyz"]
        runs = settings_of(golden, name)
        assert runs[:2] == [(0.3, 16), (0.1, 8)] and (x.shape[1] > 257 or runs[2:] == [(0.3, 64)])
        for radius, nsample in runs:
            want = golden[f"{name}_{tag(radius, nsample)}_idx"].astype(np.int32)
            t = GR.ball_group(x, None, radius, nsample)
            clear = ~t["border"]
            frac = 1.0 - clear.mean()
            print(f"{name} {tag(radius, nsample)}: borderline rows {frac:.4%}, truncated rows {(t['found'] == nsample).mean():.1%}, "
                  f"differing rows {(t['idx'] != want).any(-1).sum()}")
            assert frac <= BORDER_MAX, (name, radius, nsample, frac)
            assert np.array_equal(t["idx"][clear], want[clear]), (name, radius, nsample)
            if name.startswith("sphere") and (radius, nsample) == (0.3, 16):
                truncated = max(truncated, (t["found"] == nsample).mean())
            key = f"{name}_{tag(radius, nsample)}_idx_noself"
            if key in golden.files:
                t0 = GR.ball_group(x, None, radius, nsample, exclude_self=False)
                assert np.array_equal(t0["idx"][clear], golden[key].astype(np.int32)[clear]), (name, radius, nsample, "noself")
    assert truncated >= 0.5


def test_twin_features_match_the_reference_run(golden):
    """dxyz bit for bit; the angles within 2^-20 rad and |d| within 3 * 2^-24 of itself (the reference's are float32)."""
    name = "sphere_b2_130"
    x, nr = golden[f"{name}_xyz"], golden[f"{name}_normals"]
    for radius, nsample in settings_of(golden, name):
        t = GR.ball_group(x, nr, radius, nsample, features=("dxyz", "ppf"))
        clear = ~t["border"]
        assert np.array_equal(t["idx"][clear], golden[f"{name}_{tag(radius, nsample)}_idx"].astype(np.int32)[clear])
        dxyz, ppf = golden[f"{name}_{tag(radius, nsample)}_dxyz"], golden[f"{name}_{tag(radius, nsample)}_ppf"]
        assert dxyz.dtype == np.float32 and np.array_equal(t["dxyz"][clear].view(np.uint32), dxyz[clear].view(np.uint32))
        ang, rel = GR.ppf_errors(ppf[clear], t["feat"][clear][..., 3:], 0)
        print(f"{name} {tag(radius, nsample)}: angle error {ang / GR.ANGLE_TOL:.3f} of its bound, |d| error {rel / GR.NORM_RTOL:.3f} of its bound")
        assert ang <= GR.ANGLE_TOL and rel <= GR.NORM_RTOL, (radius, nsample, ang, rel)
        pad = np.arange(nsample)[None, None, :] >= t["found"][..., None]
        assert (t["feat"][pad] == 0).all() and (ppf[pad & clear[..., None]] == 0).all()  # pad slots: exact zeros


def loop_twin(x, radius, nsample, exclude_self, qi_list):
    """The rule as a plain loop over candidates, for one cloud."""
    r2 = float(GR.r2_of(radius))
    out = []
    for i in qi_list:
        mem = []
        for j in range(len(x)):
            dx, dy, dz = (float(x[i, c]) - float(x[j, c]) for c in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            if d <= r2 and not (exclude_self and j == i):
                mem.append(j)
        pad = i if exclude_self else (mem[0] if mem else i)
        out.append((mem[:nsample] + [pad] * nsample)[:nsample] + [min(len(mem), nsample)])
    return np.array(out)


@pytest.mark.parametrize("exclude_self", [True, False])
def test_twin_against_a_plain_loop(exclude_self):
    rs = np.random.default_rng(5)
    x = rs.uniform(-1, 1, (2, 70, 3)).astype(np.float32)
    x[0, 40] = x[0, 3]          # a duplicate is a member of its twin's row
    x[1, 7, 1] = np.nan         # a NaN point is a member of no row, and its own row is all pad
    q = np.array([[3, 40, 69, 0, 12], [7, 8, 0, 69, 33]])
    for radius, nsample in ((0.0, 2), (0.25, 4), (0.6, 8), (4.0, 64)):
        t = GR.ball_group(x, None, radius, nsample, exclude_self=exclude_self)
        tq = GR.ball_group(x, None, radius, nsample, query_idx=q, exclude_self=exclude_self)
        for b in range(2):
            want = loop_twin(x[b], radius, nsample, exclude_self, range(70))
            assert np.array_equal(t["idx"][b], want[:, :-1]) and np.array_equal(t["found"][b], want[:, -1])
            assert np.array_equal(tq["idx"][b], want[q[b], :-1]) and np.array_equal(tq["found"][b], want[q[b], -1])
        assert (t["idx"][1] != 7).sum() >= 69 * nsample and t["found"][1, 7] == 0 and (t["idx"][1, 7] == 7).all()
    dup = GR.ball_group(x, None, 0.0, 2)
    assert dup["found"][0, 3] == 1 and dup["idx"][0, 3, 0] == 40 and dup["found"][0, 40] == 1 and dup["idx"][0, 40, 0] == 3
    # ragged: rows beyond the counts are zero, a sample is its own B = 1 call, an empty sample has no rows
    r = GR.ball_group(x, None, 0.6, 8, counts=[33, 0], qcounts=[20, 5])
    own = GR.ball_group(x[:1, :33], None, 0.6, 8)
    assert np.array_equal(r["idx"][0, :20], own["idx"][0, :20]) and not r["idx"][0, 20:].any() and not r["idx"][1].any() and not r["found"][1].any()


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def call(lib, **over):
    a = dict(pts=FAKE, normals=FAKE, counts=None, query_idx=None, qcounts=None, r2=0.09, nsample=64, exclude_self=1, channels=7,
             idx=FAKE, found=FAKE, feat=FAKE, B=2, n=130, S=130)
    a.update(over)
    return lib.rrl_ball_group(a["pts"], a["normals"], a["counts"], a["query_idx"], a["qcounts"], a["r2"], a["nsample"], a["exclude_self"],
                              a["channels"], a["idx"], a["found"], a["feat"], a["B"], a["n"], a["S"], None)


REFUSALS = [dict(pts=None), dict(idx=None), dict(found=None), dict(B=0), dict(B=-1), dict(B=32768), dict(n=0), dict(S=-1), dict(S=131),
            dict(nsample=0), dict(nsample=65), dict(nsample=-1), dict(r2=-1e-9), dict(r2=float("nan")), dict(normals=None),
            dict(normals=None, channels=4), dict(channels=8), dict(channels=-1), dict(feat=None), dict(channels=0), dict(n=(1 << 20) + 1)]


def test_c_refusals_return_e_arg_without_a_launch(lib):
    assert lib.rrl_sort_capacity() == 1 << 20
    for over in REFUSALS:
        assert call(lib, **over) == E_ARG, over
    assert call(lib, S=131, n=131, B=32768) == E_ARG
    # admitted shapes that launch nothing: no queries
    assert call(lib, S=0) == 0 and call(lib, S=0, normals=None, channels=3) == 0 and call(lib, S=0, channels=0, feat=None, normals=None) == 0


def test_entry_in_the_header_and_the_binding(lib):
    from rrl_hip import _lib, build, callsites, neighbors
    assert "rrl_group.hip" in build.SOURCES and "-ffp-contract=off" in build.FLAGS
    for name, value in (("XYZ", 1), ("DXYZ", 2), ("PPF", 4), ("MAX_SAMPLE", 64)):
        assert getattr(_lib, "GROUP_" + name) == value
    assert callable(neighbors.ball_query) and callable(neighbors.ball_group)
    assert callable(callsites.rpm_sample_and_group_multi) and callable(callsites.rpm_raw_features)
    assert neighbors.FEATURES == GR.FEATURES and neighbors.FEATURE_SIZES == GR.SIZES and neighbors.MAX_NSAMPLE == 64


def test_python_refusals_need_no_gpu():
    from rrl_hip import neighbors
    x = torch.zeros(2, 6, 3)
    for kw, match in ((dict(nsample=0), "nsample"), (dict(nsample=65), "nsample"), (dict(nsample=2.5), "nsample"),
                      (dict(radius=-0.1), "radius"), (dict(radius=float("nan")), "radius"),
                      (dict(counts=[7, 1]), r"\[0, 6\]"), (dict(counts=[-1, 1]), r"\[0, 6\]"), (dict(counts=[1]), "counts"),
                      (dict(qcounts=[1, 7]), r"\[0, 6\]"), (dict(query_idx=torch.tensor([[0, 6], [0, 0]])), "query_idx"),
                      (dict(query_idx=torch.tensor([[0, -1], [0, 0]])), "query_idx"), (dict(query_idx=torch.tensor([[0, 1]])), "query_idx"),
                      (dict(query_idx=torch.tensor([[0, 3], [0, 0]]), counts=[3, 6]), "its sample's count"),
                      (dict(query_idx=torch.tensor([[0, 1], [0, 0]]), qcounts=[3, 0]), r"\[0, 2\]")):
        args = dict(radius=0.3, nsample=4)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            neighbors.ball_query(x, args.pop("radius"), args.pop("nsample"), **args)
    with pytest.raises(ValueError, match="normals"):
        neighbors.ball_group(x, None, 0.3, 4)
    with pytest.raises(ValueError, match="normals"):
        neighbors.ball_group(x, None, 0.3, 4, features=("ppf",))
    with pytest.raises(ValueError, match="normals"):
        neighbors.ball_group(x, torch.zeros(2, 5, 3), 0.3, 4)
    for bad in ((), ("xyz", "xyz"), ("normals",)):
        with pytest.raises(ValueError, match="features"):
            neighbors.ball_group(x, x, 0.3, 4, features=bad)
    with pytest.raises(ValueError, match="points"):
        neighbors.ball_query(torch.zeros(6, 3), 0.3, 4)
    with pytest.raises(ValueError, match="at least one point"):
        neighbors.ball_query(torch.zeros(2, 0, 3), 0.3, 4)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal of a machine without a GPU")
def test_without_a_gpu_the_call_raises():
    from rrl_hip import callsites, neighbors
    from rrl_hip._lib import RRLError
    x = torch.zeros(1, 4, 3)
    with pytest.raises(RRLError):
        neighbors.ball_query(x, 0.3, 4)
    with pytest.raises(RRLError):
        callsites.rpm_raw_features(x, x, ("xyz", "dxyz", "ppf"), nsample=4)
    with pytest.raises(RRLError):
        callsites.rpm_sample_and_group_multi(x, x, nsample=4)
