"""The synthetic ragged batches of tests/test_gpu_ragged.py, built on the host from seeds so that tests/test_ragged_host.py
can show with the CPU oracle that they are not vacuous (every sample that has triangles in both clouds and more than one
line populates at least one bucket).

A sample (seed, n, m, nl) is `synth.make_pair(seed, max(n, 3), max(m, 3))` -- a pseudo-triangle needs its two neighbours
-- truncated to its first n source and m target triangles, with nl lines from the reference's rejection sampler on the
generated clouds (`oracle.resample_lines(synth.uniform_streams(stream, 10, nl), ...)`; unfilled rows stay all-zero, which
are lines too).  A batch packs its samples front-aligned into (B, capN, 9), (B, capM, 9), (B, capL, 6)."""
import numpy as np

# name -> (capN, capM, capL, [(n, m, nl)]): sample b uses seed 100 + b and line stream b.
# BASE: eight pairs of very different sizes, 2048 lines each (the "absent rows" and deterministic tests).
# TAIL / TILE / XCHG: the three shapes of DESIGN section 3's shape -> kernel table (a step's backward in the tail kernel; one
# tile of lines with the chunked sort beyond 4096 triangles; the exchange reduce beyond 256 (sample, tile) pairs), with
# counts that include 0, 1, 63, 64, 65 and the capacity and line counts that include 0, 1, 1023, 1024, 1025 and the capacity.
BATCHES = {
    "BASE": (2048, 2048, 2048, [(64, 2048, 2048), (257, 1500, 2048), (1000, 333, 2048), (1777, 2048, 2048), (2048, 65, 2048),
                                (130, 129, 2048), (1, 2048, 2048), (2048, 2048, 2048)]),
    "TAIL": (4096, 4096, 10000, [(4096, 4096, 10000), (0, 2048, 3000), (1, 2048, 2048), (63, 3000, 1023), (64, 1, 1024),
                                 (65, 4096, 1025), (2048, 0, 0), (3000, 65, 1)]),
    "TILE": (16384, 16384, 512, [(16384, 16384, 512), (0, 64, 0), (63, 4097, 511), (65, 1, 512)]),
    "XCHG": (1024, 1024, 10000, [(1024, 1024, 10000), (0, 700, 2000), (1, 1024, 2048), (63, 900, 1023), (64, 64, 1024),
                                 (65, 1, 1025), (1024, 0, 1500), (700, 65, 1), (512, 300, 0)] +
             [(40 + 41 * b, 1024 - 37 * b, 1200 + 130 * b) for b in range(23)]),
}
assert len(BATCHES["XCHG"][3]) == 32 and len(BATCHES["TAIL"][3]) == 8

_cache = {}


def sample(oracle, seed, stream, n, m, nl):
    """dict(tri1 (n, 9), tri2 (m, 9), lines (nl, 6)) of one sample."""
    from rrl_hip import synth
    p = synth.make_pair(seed, max(n, 3), max(m, 3))
    lines = np.zeros((0, 6), np.float32)
    if nl > 0:
        lines = oracle.resample_lines(synth.uniform_streams(stream, 10, nl), p["radius"], p["center"], p["src"], p["tar"], nl)
    return dict(tri1=np.ascontiguousarray(p["src_tri"][:n]), tri2=np.ascontiguousarray(p["tar_tri"][:m]),
                lines=np.ascontiguousarray(lines, np.float32))


def batch(oracle, name):
    """(capN, capM, capL, [sample dicts]) of a named batch (cached per process)."""
    if name not in _cache:
        capN, capM, capL, rows = BATCHES[name]
        _cache[name] = (capN, capM, capL, [sample(oracle, 100 + b, b, n, m, nl) for b, (n, m, nl) in enumerate(rows)])
    return _cache[name]


def may_be_empty(s):
    """A sample that is allowed to have no populated bucket: a cloud without triangles, or at most one line."""
    return len(s["tri1"]) == 0 or len(s["tri2"]) == 0 or len(s["lines"]) <= 1


def packed(oracle, name, fill=float("nan")):
    """The batch as capacity-shaped numpy arrays (absent rows = fill) + counts: (p1, p2, ln, c1, c2, nl, samples)."""
    capN, capM, capL, ss = batch(oracle, name)
    B = len(ss)
    p1 = np.full((B, capN, 9), fill, np.float32)
    p2 = np.full((B, capM, 9), fill, np.float32)
    ln = np.full((B, capL, 6), fill, np.float32)
    for b, s in enumerate(ss):
        p1[b, :len(s["tri1"])] = s["tri1"]
        p2[b, :len(s["tri2"])] = s["tri2"]
        ln[b, :len(s["lines"])] = s["lines"]
    c1 = np.array([len(s["tri1"]) for s in ss], np.int32)
    c2 = np.array([len(s["tri2"]) for s in ss], np.int32)
    nl = np.array([len(s["lines"]) for s in ss], np.int32)
    return p1, p2, ln, c1, c2, nl, ss


# The step / filler / graph tests: BASE's clouds with UNEVEN line counts; step `it` gives sample b the first STEP_NL[b] lines of
# sample (b + it) % B (new lines in every step).  GRAPH_VARIANTS: the (counts1, nlines) a captured step is replayed with.
STEP_NL = [2048, 1500, 1025, 1024, 1023, 2048, 2048, 700]
GRAPH_VARIANTS = [([64, 257, 1000, 1777, 2048, 130, 1, 2048], STEP_NL),
                  ([64, 128, 1000, 888, 2048, 65, 1, 1024], [700, 2048, 1023, 64, 1500, 1, 2000, 2048]),
                  ([64, 257, 1000, 1777, 2048, 130, 1, 2048], [700, 2048, 1023, 64, 1500, 1, 2000, 2048])]


HALF_C2 = [1024, 750, 166, 1024, 32, 64, 1024, 1024]  # half of BASE's target counts (a new counts2 is a new target)


def step_samples(oracle, it, counts1=None, nlines=None, counts2=None):
    """The sample dicts of step `it` (optionally with other source counts / line counts: GRAPH_VARIANTS; target counts)."""
    _, _, _, ss = batch(oracle, "BASE")
    B = len(ss)
    nlines = STEP_NL if nlines is None else nlines
    return [dict(tri1=s["tri1"] if counts1 is None else s["tri1"][:counts1[b]],
                 tri2=s["tri2"] if counts2 is None else s["tri2"][:counts2[b]],
                 lines=ss[(b + it) % B]["lines"][:nlines[b]]) for b, s in enumerate(ss)]


def packed_step(oracle, it, fill=float("nan")):
    """packed() for step `it`: capacities 2048 / 2048 / 2048."""
    ss = step_samples(oracle, it)
    p1, p2, _, c1, c2, _, _ = packed(oracle, "BASE", fill)
    ln = np.full((len(ss), 2048, 6), fill, np.float32)
    for b, s in enumerate(ss):
        ln[b, :len(s["lines"])] = s["lines"]
    return p1, p2, ln, c1, c2, np.array(STEP_NL, np.int32), ss


# The reference's own pairs as ONE batch (test 1): capacities 2048 / 2048 / 3000.
REF_NAMES = ["ref_airplane%d" % i for i in range(5)] + ["ref_human%d" % i for i in range(3)] + ["ref_real%d" % i for i in range(3)] + \
    ["synth_s0", "synth_s1", "edge_zero_dup", "edge_allmiss"]
