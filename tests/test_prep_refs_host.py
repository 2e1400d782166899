"""CPU-side check of tests/prep_refs.py: the twins that tests/test_gpu_prep_kernels.py holds the cloud-preparation and
line-drawing kernels to are right by themselves -- Philox4x32-10 reproduces the published Random123 known answers, fps_ref
followed by knn3_ref reproduces the reference's recorded Sample_neighs rows bit for bit, candidate_ref reproduces the
reference's recorded candidates within the one bound, and the pinned corner cases (the 1e10 cap, index 0 repeating once
every distance is zero, ties to the lower index) are what the twins do.  Plus the host-side argument checks of
rrl_hip.neighbors, which must refuse a bad index BEFORE any launch."""
import numpy as np
import pytest
import torch

import prep_refs as PF
from conftest import load_golden


# ----------------------------------------------------------------------------------------------------------------- Philox
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    """The three known-answer vectors of Random123's kat_vectors for philox4x32 with 10 rounds."""
    got = PF.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(x) for x in got) == want


def test_philox_broadcasts_and_sampler_uniforms_use_every_counter_word():
    """Arrays give the scalars' answers element by element; the uniforms are 24-bit values in [0, 1), and changing any one
    of candidate, round, sample, either half of the call number or either half of the seed changes them."""
    i = np.arange(5)
    blk = PF.philox4x32_10((i, 7, 8, 9), (10, 11))
    for j in i:
        np.testing.assert_array_equal(blk[:, j], PF.philox4x32_10((int(j), 7, 8, 9), (10, 11)))
    seed, call = PF.RNG_SEEDS[1], PF.RNG_HIGH_CALL
    base = PF.sampler_uniforms(seed, call, 2, 3, np.arange(1000))
    assert base.dtype == np.float32 and base.shape == (4, 1000) and base.min() >= 0.0 and base.max() < 1.0
    np.testing.assert_array_equal(base * 2.0 ** 24, np.round(base * 2.0 ** 24))
    assert abs(float(base.mean()) - 0.5) < 0.02
    x = PF.philox4x32_10((np.arange(1000), 3 | (2 << 16), call & 0xffffffff, call >> 32), (seed & 0xffffffff, seed >> 32))
    np.testing.assert_array_equal(base, ((x >> 8) / 2.0 ** 24).astype(np.float32))
    others = [PF.sampler_uniforms(seed, call, 2, 3, np.arange(1000) + 1000), PF.sampler_uniforms(seed, call, 2, 4, np.arange(1000)),
              PF.sampler_uniforms(seed, call, 1, 3, np.arange(1000)), PF.sampler_uniforms(seed, call + 1, 2, 3, np.arange(1000)),
              PF.sampler_uniforms(seed, call - 2 ** 32, 2, 3, np.arange(1000)), PF.sampler_uniforms(seed + 1, call, 2, 3, np.arange(1000)),
              PF.sampler_uniforms(seed & 0xffffffff, call, 2, 3, np.arange(1000))]
    for o in others:
        assert np.count_nonzero(o == base) < 10


# ----------------------------------------------------------------------------------------------------------------- FPS, 3-NN
@pytest.mark.parametrize("seed, S, key", [(77, 900, "full"), (78, 300, "sub")])
def test_twins_reproduce_the_reference_sample_neighs(seed, S, key):
    """tests/golden/sample_neighs.npz (the reference's Sample_neighs, code/loss.py:473-485, on 900 points): the start index
    from torch's CPU generator like the reference draws it, fps_ref, knn3_ref -- the same rows, bit for bit."""
    g = load_golden("sample_neighs.npz")
    pts = g["points"]
    torch.manual_seed(seed)
    start = int(torch.randint(0, len(pts), (1,)))
    idx = PF.fps_ref(pts, S, start)
    assert idx[0] == start and len(set(idx.tolist())) == S
    nn = PF.knn3_ref(pts, idx)
    np.testing.assert_array_equal(nn[:, 0], idx)  # (no duplicates in this cloud: every query is its own nearest point)
    rows = pts[nn.reshape(-1)]
    assert rows.shape == g[key].shape
    np.testing.assert_array_equal(rows.view(np.uint32), g[key].view(np.uint32))


def test_fps_ref_cap_ties_squared_distances_above_1e10():
    """Coordinates of order 2e5: most squared distances exceed 1e10, stay AT the cap after the minimum, and tie -- the
    second sample is the first point farther than 1e5 from the start, not the farthest one."""
    p = PF.far_cloud(41)
    s = PF.sq_dist(p, p[5])
    assert np.count_nonzero(s > PF.FPS_CAP) > len(p) // 2
    idx, dist = PF.fps_ref(p, PF.FAR_S, 5, return_dist=True)
    assert idx[1] == int(np.argmax(s >= PF.FPS_CAP)) and idx[1] != int(np.argmax(s))
    assert dist.max() <= PF.FPS_CAP and len(set(idx.tolist())) == PF.FAR_S


def test_fps_ref_repeats_index_0_once_every_distance_is_zero():
    """The lattice with copies: 1728 distinct positions among 2028 points.  The first 1728 samples take every position once
    (the lower index of a point and its copy), then every distance is 0 and argmax gives index 0 for the rest."""
    p = PF.lattice_cloud(43)
    assert p.shape == (PF.LATTICE_SIDE ** 3 + PF.LATTICE_COPIES, 3)
    idx, dist = PF.fps_ref(p, len(p), 17, return_dist=True)
    k = PF.LATTICE_SIDE ** 3
    assert len({tuple(r) for r in p[idx[:k]]}) == k and idx[:k].max() < k
    np.testing.assert_array_equal(idx[k:], 0)
    assert not dist.any()


def test_knn3_ref_ties_go_to_the_lower_index():
    """On the lattice a copy at a higher index finds its twin FIRST, then itself; neighbours at distance 1 come in index
    order; a stable sort over float64 distances is an exhaustive (distance, index) order."""
    p = PF.lattice_cloud(43)
    k = PF.LATTICE_SIDE ** 3
    q = np.concatenate([np.arange(k, k + 40), np.arange(0, 200)])
    nn = PF.knn3_ref(p, q)
    d2 = ((p[q][:, None, :].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(-1)
    for row, (qi, n3) in enumerate(zip(q, nn)):
        order = sorted(range(len(p)), key=lambda j: (d2[row, j], j))[:3]
        assert list(n3) == order
        assert d2[row, n3[0]] == 0.0
    copies = nn[:40]
    assert np.all(copies[:, 0] < k) and np.all(copies[:, 0] != q[:40])  # "itself first" is false for a copy
    assert np.all((copies[:, 1] == q[:40]) | (d2[np.arange(40), copies[:, 1]] == 0.0))


def test_aabb_ref_is_min_and_max():
    v = PF.gaussian_cloud(1, 2, 50)
    v[1, 7, 2] = np.inf
    r = PF.aabb_ref(v)
    assert r.shape == (2, 6) and r[1, 5] == np.inf
    for b in range(2):
        for c in range(3):
            assert r[b, c] == min(v[b, :, c]) and r[b, 3 + c] == max(v[b, :, c])


# ----------------------------------------------------------------------------------------------------------------- candidates
def test_candidate_ref_reproduces_the_reference_candidates():
    """tests/golden/sampler.npz: cand0 is what the reference (torch on the CPU, float32) made of round 0 of `rands`.  It lies
    within the device's bound of the float64 twin -- and so, by construction, does the float32 twin."""
    g = load_golden("sampler.npz")
    u = np.ascontiguousarray(g["rands"][0])
    cb = PF.candidate_bound(u, g["radius"], g["center"])
    assert cb["left_out"] <= PF.SHORT_CHORD_CAP
    host, _ = PF.candidate_ref(u, g["radius"], g["center"], np.float32)
    assert host.dtype == np.float32
    for name, lines in (("reference", g["cand0"]), ("float32 twin", host)):
        ed, eo = PF.candidate_errors(lines, cb)
        print(f"{name}: direction {ed:.2e} (bound {cb['bound'][0]:.2e}), origin {eo:.2e} (bound {cb['bound'][1]:.2e})")
        assert ed <= cb["bound"][0] and eo <= cb["bound"][1]
    # the bound discriminates: a neighbouring candidate's uniforms move a line by order radius
    ed, eo = PF.candidate_errors(np.roll(g["cand0"], 1, axis=0), cb)
    assert ed > 1e4 * cb["bound"][0] and eo > 1e4 * cb["bound"][1]


def test_candidate_yardstick_at_the_gpu_tests_shapes():
    """The float32 host error on 200 000 twin candidates is of the order of a few float32 roundings (so 4 x it is no
    loophole), the share of short chords is the 0.05^2 / 4 of two uniform points on a sphere, the lines are unit directions
    through points on the sphere, and chords and radii scale together."""
    u = PF.sampler_uniforms(PF.RNG_SEEDS[0], 0, 0, 0, np.arange(200000))
    cb = PF.candidate_bound(u, 1.7, PF.CAND_CENTRES[1])
    print(f"float32 host error on 200 000 candidates at radius 1.7: direction {cb['host'][0]:.2e}, origin {cb['host'][1]:.2e}; "
          f"short chords {cb['left_out']:.6f}")
    assert cb["host"][0] < 2e-5 and cb["host"][1] < 4e-6
    assert abs(cb["left_out"] - PF.SHORT_CHORD ** 2 / 4) < 3e-4
    ref, chord = PF.candidate_ref(u, 1.7, PF.CAND_CENTRES[1], np.float64)
    np.testing.assert_allclose(np.linalg.norm(ref[:, :3], axis=1), 1.0, atol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(ref[:, 3:] - PF.CAND_CENTRES[1].astype(np.float64), axis=1), float(np.float32(1.7)), rtol=1e-7)
    x0 = (ref[:, 3:] - PF.CAND_CENTRES[1].astype(np.float64)) / float(np.float32(1.7))
    assert np.abs(x0.mean(0)).max() < 0.01 and np.abs((x0 ** 2).mean(0) - 1 / 3).max() < 0.01
    _, chord2 = PF.candidate_ref(u, 3.4, PF.CAND_CENTRES[2], np.float64)
    np.testing.assert_allclose(chord2, 2 * chord, rtol=1e-6)


# ----------------------------------------------------------------------------------------------------------------- validation
@pytest.fixture
def no_launch(monkeypatch):
    """rrl_hip.neighbors with its launcher replaced: reaching it fails the test, so a bad index can never reach a device."""
    from rrl_hip import neighbors

    def reached(*a, **k):
        pytest.fail(f"a launch was reached: {a[1] if len(a) > 1 else a}")
    monkeypatch.setattr(neighbors, "_run", reached)
    return neighbors


@pytest.mark.parametrize("start", [[-1, 0], [0, 50], [50, 0], [2 ** 31, 0], [0], [0, 1, 2]])
def test_fps_refuses_a_start_outside_the_cloud(no_launch, start):
    """start outside [0, n), or not one per cloud: ValueError before any launch (the kernel reads pts[3 start])."""
    pts = torch.zeros(2, 50, 3)
    with pytest.raises(ValueError, match="start"):
        no_launch.fps(pts, 10, start=torch.tensor(start))


@pytest.mark.parametrize("query", [[[0, 50]], [[-1, 3]], [[2 ** 31 + 1, 3]]])
def test_knn3_refuses_a_query_outside_the_cloud(no_launch, query):
    pts = torch.zeros(1, 50, 3)
    with pytest.raises(ValueError, match="query_idx"):
        no_launch.knn3(pts, torch.tensor(query))


@pytest.mark.parametrize("n", [1, 2])
def test_knn3_and_sample_neighs_refuse_fewer_than_three_points(no_launch, n):
    """Three neighbours of fewer than three points do not exist (the reference's KDTree.query(k=3) raises)."""
    with pytest.raises(ValueError, match="3 points"):
        no_launch.knn3(torch.zeros(1, n, 3), torch.zeros(1, 1, dtype=torch.long))
    with pytest.raises(ValueError, match="3 points"):
        no_launch.sample_neighs(np.zeros((n, 3), np.float32))
