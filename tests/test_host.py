"""CPU-side checks: the C-ABI library loads and validates its arguments (its exports and the binding's agreement with
include/rrl.h: tests/test_abi_host.py), host logic (LieAlgebra, utils, synth), and loud failure without a GPU.  No compute calls."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def libpath():
    from rrl_hip import build
    return build.build_lib()  # hipcc cross-compiles gfx950 without a GPU


def test_abi_argument_errors(libpath):
    """Argument validation happens on the host before any HIP call."""
    from rrl_hip import _lib
    lib = _lib.load()
    assert lib.rrl_tri_prepare(None, None, None, 0, 1, 1, 1, 1, None) == -1
    assert lib.rrl_set_scan_variant(3) == -1
    assert lib.rrl_rigid_bwd_blocks(5000) == 1 and lib.rrl_rigid_bwd_blocks(40000) == 3
    assert lib.rrl_loss_reduce(None, 0, None, 1, 1, 1, 1, 1, 1, 5, 5, 0, None) == -1
    # workspace layout: 256-byte aligned, monotone, inside the reported size
    import ctypes as C
    from rrl_hip import ops
    names = table_names("WS")
    assert [n.upper() for n in field_names(lib, 0)] == names  # the library describes the header's table, in order
    assert [n.upper() for n in field_names(lib, 1)] == table_names("WW")
    assert len(names) == len(ops._WS.index) == 52 and len(ops._WW.index) == 16
    n_fields = len(names)
    offs = (C.c_size_t * n_fields)()
    assert lib.rrl_workspace_layout(8, 4096, 4096, 10000, offs) == 0
    total = lib.rrl_workspace_bytes(8, 4096, 4096, 10000)
    o = [int(v) for v in offs]
    assert o[0] == 0 and o == sorted(o) and all(v % 256 == 0 for v in o) and o[-1] < total
    assert total < 64 << 20
    # rrl_workspace_field: unknown kind / field refused, every output optional
    shape = (8, 4096, 4096, 10000, 8)
    name, code, dims = C.c_char_p(), C.c_int(), (C.c_longlong * 4)()
    for kind, field in ((2, 0), (-1, 0), (0, -2), (0, 52), (1, 16), (1, -2)):
        assert lib.rrl_workspace_field(kind, field, *shape, C.byref(name), C.byref(code), dims) == -1, (kind, field)
    assert lib.rrl_workspace_field(0, -1, *shape, None, None, None) == 52
    assert lib.rrl_workspace_field(1, -1, *shape, None, None, None) == 16
    assert lib.rrl_workspace_field(0, 6, *shape, None, None, None) == 3  # HIT1 [B][L][4]
    assert lib.rrl_workspace_field(0, 6, *shape, C.byref(name), C.byref(code), dims) == 3
    assert (name.value, code.value, list(dims)[:3]) == (b"hit1", 1, [8, 10000, 4])


def table_names(kind):
    """The field names of include/rrl.h's RRL_<kind>_TABLE, in order."""
    header = open(os.path.join(ROOT, "include", "rrl.h")).read()
    table = header[header.index(f"#define RRL_{kind}_TABLE(X)"):header.index(f"#define RRL_{kind}_ENUM_")]
    return re.findall(r"\bX\(([A-Z0-9]+),", table)


def field_names(lib, kind):
    import ctypes as C
    out = []
    for i in range(lib.rrl_workspace_field(kind, -1, 0, 0, 0, 0, 0, None, None, None)):
        name = C.c_char_p()
        assert 1 <= lib.rrl_workspace_field(kind, i, 0, 0, 0, 0, 0, C.byref(name), None, None) <= 4
        out.append(name.value.decode())
    return out


def test_layout_and_views_reproduce_the_recorded_fixture(libpath):
    """tests/golden/ws_layout.json was recorded from the hand-written size and view tables that the field tables of
    include/rrl.h replaced (its "generator" key holds the script): totals, offsets, and every view's name, dtype and shape
    at G = 1 and G = B are reproduced exactly by the library and rrl_hip.ops at all twelve shapes, and every view ends at
    or before the next field's offset.  (B = 0 has G = 0 only: G <= B.  A negative extent: the layout entries refuse, so
    no state exists; the fixture pins the refusal and the clamped total.)"""
    import ctypes as C
    import json
    from rrl_hip import RRLError, _lib, ops
    lib = _lib.load()
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "ws_layout.json")))
    assert len(fixture["cases"]) == 12
    for case in fixture["cases"]:
        shape = tuple(case["shape"])
        for key, W in (("ws", ops._WS), ("wws", ops._WW)):
            want, names = case[key], list(W.index)
            offs = (C.c_size_t * len(names))()
            assert getattr(lib, W.entry + "_layout")(*shape, offs) == want["layout_rc"], (shape, key)
            total = int(getattr(lib, W.entry + "_bytes")(*shape))
            assert total == want["total"], (shape, key)
            if want["layout_rc"]:
                with pytest.raises(RRLError):
                    W.spec(shape + (1,), names[0])
                continue
            assert [int(o) for o in offs] == want["offsets"] == W.layout(*shape)[1] and W.layout(*shape)[0] == total, (shape, key)
            ends = want["offsets"][1:] + [total]
            groups = sorted({min(1, shape[0]), shape[0]})
            assert sorted(k for k in want if k.startswith("views_G")) == sorted(f"views_G{G}" for G in groups)
            for G in groups:
                specs = [W.spec(shape + (G,), n) for n in names]
                got = [[n, str(dt).split(".")[1], list(shp)] for n, (_, _, dt, shp) in zip(names, specs)]
                assert got == want[f"views_G{G}"], (shape, key, G)
                for i, (off, nbytes, _, _) in enumerate(specs):
                    assert off == want["offsets"][i] and off + nbytes <= ends[i], (shape, key, G, names[i])


def test_no_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import loss
    from rrl_hip import RRLError
    with pytest.raises(RRLError, match="no CPU fallback"):
        loss.chamfer_dist(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))
    with pytest.raises(RRLError):
        loss.cal_loss_intersection_batch_whole_median_pts_lines(
            1, 1, 5, 5, torch.zeros(1, 4, 9), torch.zeros(1, 4, 9), torch.zeros(1, 8, 6))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "a-robust-registration-loss_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "rrl_oracle" not in text and "import oracle" not in text, f
    # developer tools time the product only; bench.py may use the oracle in its cpu_baseline leg alone
    for dirpath, _, files in os.walk(os.path.join(ROOT, "tools")):  # (tools/attic too)
        for f in files:
            text = open(os.path.join(dirpath, f), errors="ignore").read()
            assert "rrl_oracle" not in text and "from oracle" not in text and "import oracle" not in text, f
    bench = open(os.path.join(ROOT, "bench.py")).read()
    # bench.py: the oracle is the CHECKER, never the thing measured -- only inside cpu_baseline() (the reported CPU leg) and
    # parity_in_run() (round 6: the oracle's check of the timed workload, run after the timed region)
    uses = [i for i in range(len(bench)) if bench.startswith("rrl_oracle", i)]
    spans = []
    for name in ("def cpu_baseline(", "def parity_in_run("):
        lo = bench.index(name)
        spans.append((lo, bench.index("\ndef ", lo + 1)))
    assert uses and all(any(lo < i < hi for lo, hi in spans) for i in uses)
    timed = bench[bench.index("    t0 = timed(step, args.steps)"):bench.index("    fence()  # closing barrier")]
    assert "oracle" not in timed and "parity_in_run" not in timed


def test_lie_algebra_vs_reference():
    from LieAlgebra import se3, so3
    g = load_golden("se3_exp_log.npz")
    xi = torch.from_numpy(g["xi"])
    R, p = se3.exp3(xi)
    np.testing.assert_allclose(R.numpy(), g["R"], atol=1e-7)
    np.testing.assert_allclose(p.numpy(), g["p"], atol=1e-7)
    np.testing.assert_allclose(se3.exp(xi).numpy(), g["g"], atol=1e-7)
    np.testing.assert_allclose(se3.log(torch.from_numpy(g["g"])).numpy(), g["log_of_exp"], atol=1e-6)
    # log(exp(xi)) == xi away from the pi branch
    np.testing.assert_allclose(se3.log(se3.exp(xi[:5])).numpy(), g["xi"][:5], atol=2e-5)
    # finite gradient at the identity (the reference's norm() gives NaN there)
    x = torch.zeros(6, requires_grad=True)
    R, p = se3.exp3(x)
    (R.sum() + p.sum()).backward()
    assert torch.isfinite(x.grad).all()
    np.testing.assert_allclose(so3.vec(so3.mat(xi[:, :3])).numpy(), g["xi"][:, :3])
    g4 = se3.exp(xi)
    eye = g4 @ se3.inverse(g4)
    np.testing.assert_allclose(eye.numpy(), np.tile(np.eye(4, dtype=np.float32), (6, 1, 1)), atol=2e-6)


def test_exp3_gradient_matches_autograd_of_reference_formula():
    from LieAlgebra import se3
    g = load_golden("reconstruction_point.npz")
    xi = torch.from_numpy(g["xi"]).requires_grad_(True)
    R, T = se3.exp3(xi)
    pts = torch.from_numpy(g["src"]) @ R[0] + T
    tri = torch.from_numpy(g["src_tri"]).reshape(-1, 3) @ R[0] + T
    ((pts * torch.from_numpy(g["g_pts"])).sum()
     + (tri.reshape(-1, 9) * torch.from_numpy(g["g_tri"])).sum()).backward()
    np.testing.assert_allclose(xi.grad.numpy(), g["grad_xi"], rtol=1e-4, atol=1e-4)


def test_utils_host_helpers(tmp_path):
    import utils
    d = {"a": torch.zeros(2), "b": 3}
    utils.dict_all_to_device(d, "cpu")
    assert d["b"] == 3 and d["a"].device.type == "cpu"
    utils.Dict2txt_json(str(tmp_path / "x.json"), {"k": 1.5}, file_type="json")
    assert open(tmp_path / "x.json").read() == '{"k": 1.5}'
    utils.Dict2txt_json(str(tmp_path / "x.txt"), {"k": 1.5, "j": 2})
    assert open(tmp_path / "x.txt").read() == "k:1.5\nj:2\n"
    utils.mkdir_ifnotexists(str(tmp_path / "sub"))
    assert os.path.isdir(tmp_path / "sub")
    v = torch.arange(24.0).reshape(1, 8, 3)
    f = torch.tensor([[[2, 0, 6], [5, 7, 6]]])
    fv = utils.makefacevertices(v, f)
    assert fv.shape == (1, 2, 9)
    np.testing.assert_array_equal(fv[0, 0].numpy(), np.concatenate([v[0, 2], v[0, 0], v[0, 6]]))
    q = torch.tensor([[0.0, 0.0, np.sin(0.25), np.cos(0.25)]])
    np.testing.assert_allclose(utils.npmat2euler(utils.quat2mat(q).numpy())[0],
                               [np.rad2deg(0.5), 0, 0], atol=1e-4)


def test_synth_is_deterministic_and_well_formed():
    from rrl_hip import synth
    a, b = synth.make_pair(3, 200, 150), synth.make_pair(3, 200, 150)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert a["src_tri"].shape == (200, 9) and a["tar_tri"].shape == (150, 9)
    np.testing.assert_array_equal(a["src_tri"][:, :3], a["src"])  # P0 is the point itself
    d1 = np.linalg.norm(a["src_tri"][:, 3:6] - a["src"], axis=1)
    d2 = np.linalg.norm(a["src_tri"][:, 6:9] - a["src"], axis=1)
    assert np.all(d1 <= d2 + 1e-7) and np.all(d1 > 0)
    c = synth.make_pair(4, 256, 128, crop=True)
    assert c["tar"].shape == (128, 3)
    r = synth.uniform_streams(5, 2, 7)
    assert r.shape == (2, 4, 7) and 0 <= r.min() and r.max() < 1


def test_stacked_rand_consumes_the_generator_like_separate_calls():
    """loss._uniform_rounds draws all rounds with ONE torch.rand: same CPU stream as the reference's
    four `torch.rand(B, n)` calls per round (code/loss.py:394-402)."""
    import torch
    for B, n, rounds in ((1, 20000, 10), (3, 777, 10), (2, 8, 3), (8, 10000, 2)):
        torch.manual_seed(11)
        seq = torch.stack([torch.stack([torch.rand(B, n) for _ in range(4)]) for _ in range(rounds)])
        torch.manual_seed(11)
        one = torch.rand(rounds, 4, B, n)
        assert torch.equal(seq, one), (B, n, rounds)


STAGE_HEADERS = ["rrl_stage_pair.h", "rrl_stage_reduce.h", "rrl_stage_tail.h", "rrl_stage_bwd.h", "rrl_stage_args.h", "rrl_stamps.h"]


@pytest.mark.parametrize("header", STAGE_HEADERS)
def test_stage_headers_stand_alone(tmp_path, header):
    """Every header of the stages behind the scan includes what it uses and needs no macro from its includer: a unit that
    holds nothing but `#include "<header>"` passes hipcc with the library's flags."""
    import subprocess
    from rrl_hip import build
    unit = tmp_path / "alone.hip"
    unit.write_text(f'#include "{os.path.join(build.CSRC, header)}"\n')
    subprocess.check_call([build._hipcc(), *build.FLAGS, "-fsyntax-only", str(unit)])


def test_control_word_map():
    """The control words of a sample's MCTL / CHAIN row have ONE map, include/rrl.h's RRL_MCTL_* / RRL_CHAIN_* enumerators:
    the values the Python binding mirrors equal it, the row lengths are the last extents of the two fields in the workspace
    table, and no two users of an MCTL word share one."""
    from rrl_hip import _abi, _lib
    header = open(os.path.join(ROOT, "include", "rrl.h")).read()
    words = _abi.CONSTANTS  # (each one against gcc's value: tests/test_abi_host.py)
    mctl ={k[len("RRL_MCTL_"):]: v for k, v in words.items() if k.startswith("RRL_MCTL_")}
    chain = {k[len("RRL_CHAIN_"):]: v for k, v in words.items() if k.startswith("RRL_CHAIN_")}
    assert set(mctl) == {"BUCKET0", "CURSOR", "TICK1", "TICK2", "ERR", "MEDBITS", "MEDRDY", "BAD", "CHAM_GROUP", "CHAM_TOP", "LSUM",
                         "WORDS"}
    assert list(chain) == ["READY", "NAN", "FALLBACK", "TIMEOUT", "WORDS"] and list(chain.values()) == [0, 1, 2, 3, 4]
    mirrored = {k: v for k, v in vars(_lib).items() if k.startswith(("MCTL_", "CHAIN_"))}
    assert mirrored and "MCTL_ERR" in mirrored
    for name, value in mirrored.items():
        assert words["RRL_" + name] == value, name
    # the rows: the last extent of the field's row in RRL_WS_TABLE
    for field, row in (("MCTL", mctl["WORDS"]), ("CHAIN", chain["WORDS"])):
        extents = re.search(r"X\(%s, int32_t, ([^)]*)\)" % field, header).group(1)
        assert int(extents.split(",")[-1]) == row, field
    # MCTL: sixteen buckets, then every user's words (two Chamfer directions, a 64-bit loss sum), distinct and inside the row
    used = [mctl[k] for k in ("CURSOR", "TICK1", "TICK2", "ERR", "MEDBITS", "MEDRDY", "BAD", "CHAM_TOP")]
    used += [mctl["CHAM_GROUP"], mctl["CHAM_GROUP"] + 1, mctl["LSUM"], mctl["LSUM"] + 1]
    used += list(range(mctl["BUCKET0"], mctl["BUCKET0"] + 16))
    assert len(set(used)) == len(used) and min(used) >= 0 and max(used) < mctl["WORDS"]
    assert mctl["LSUM"] % 2 == 0
