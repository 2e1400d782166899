"""Guard bands, field extents and an allocation seam for the workspace tests (tests/test_ws_layout_host.py,
tests/test_gpu_workspace.py).  Imported like loss_refs.py; no fixture, no conftest.

The loss pipeline computes in caller-allocated workspaces (include/rrl.h RRL_WS_TABLE / RRL_WW_TABLE) and scratches that
rrl_hip.ops takes from torch.empty.  Three things are provided here:

  * guarded / bands_intact: a buffer with `band` bytes of a fill pattern in front of and behind its middle;
  * field_extents / gaps / clear_spans: where the library says the fields lie (rrl_workspace_layout /
    rrl_wide_workspace_layout for the offsets, rrl_workspace_field for the extents -- nothing from the Python views' cached
    specs), the bytes that belong to no field, and the spans the host code clears with ONE fill across field boundaries
    (csrc/rrl_ws.h's static_asserts): padding inside such a span may be zeroed, padding anywhere else must never be written;
  * Arena: while `with arena.patch(ops)` is active every device buffer rrl_hip.ops allocates (torch.empty / empty_like /
    zeros: workspaces, scratches, losses, gradients, keys, orders) is the middle of a guarded buffer pre-filled with the
    arena's fill.  ops builds its call records from these tensors, so the steps' baked-in pointers point into guarded memory
    without a seam in ops.py.  arena.recycle() hands the workspaces and scratches of the evaluations made so far to the next
    allocations of the same size AS THEY ARE: the "dirty" prior content of a call that must assume nothing.
"""
import contextlib
import ctypes

import torch

BAND = 4096
_ITEM = (1, 4, 4, 8)  # include/rrl.h RRL_T_U8, RRL_T_I32, RRL_T_F32, RRL_T_I64
_LAYOUT = ("rrl_workspace", "rrl_wide_workspace")


def guarded(nbytes, fill, band=BAND, device="cuda"):
    """(buf, middle): one uint8 device buffer of band + nbytes + band bytes, all `fill`, and the view of its middle nbytes
    (band is a multiple of 256: the middle keeps the allocation's alignment)."""
    assert band % 256 == 0 and 0 <= fill <= 255
    buf = torch.full((band + nbytes + band,), fill, dtype=torch.uint8, device=device)
    return buf, buf[band:band + nbytes]


def bands_intact(buf, nbytes, fill, band=BAND):
    """True when both bands of a guarded buffer still hold `fill`."""
    assert buf.numel() == band + nbytes + band
    return bool((buf[:band] == fill).all()) and bool((buf[band + nbytes:] == fill).all())


def _lib():
    from rrl_hip import _lib
    return _lib.load()


def workspace_bytes(kind, B, N, M, L):
    return int(getattr(_lib(), _LAYOUT[kind] + "_bytes")(B, N, M, L))


def field_extents(kind, B, N, M, L, G):
    """[(name, offset, bytes)] of workspace `kind` (0: RRL_WS_TABLE, 1: RRL_WW_TABLE) at shape (B, N, M, L) with G groups,
    in table order: the offset from the layout entry, the bytes from rrl_workspace_field's element type and extents."""
    lib = _lib()
    n = lib.rrl_workspace_field(kind, -1, 0, 0, 0, 0, 0, None, None, None)
    assert n > 0
    offs = (ctypes.c_size_t * n)()
    rc = getattr(lib, _LAYOUT[kind] + "_layout")(B, N, M, L, offs)
    assert rc == 0, (kind, B, N, M, L, rc)
    out = []
    for i in range(n):
        name, code, dims = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_longlong * 4)()
        rank = lib.rrl_workspace_field(kind, i, B, N, M, L, G, ctypes.byref(name), ctypes.byref(code), dims)
        assert 1 <= rank <= 4, (kind, i, rank)
        nbytes = _ITEM[code.value]
        for d in dims[:rank]:
            nbytes *= int(d)
        out.append((name.value.decode(), int(offs[i]), nbytes))
    return out


def element_sizes(kind):
    """{field name: bytes of one element} of workspace `kind`."""
    lib = _lib()
    out = {}
    for i in range(lib.rrl_workspace_field(kind, -1, 0, 0, 0, 0, 0, None, None, None)):
        name, code = ctypes.c_char_p(), ctypes.c_int()
        lib.rrl_workspace_field(kind, i, 0, 0, 0, 0, 0, ctypes.byref(name), ctypes.byref(code), None)
        out[name.value.decode()] = _ITEM[code.value]
    return out


def gaps(extents, nbytes):
    """[(lo, hi)]: the byte ranges of [0, nbytes) that belong to no field -- the padding behind every field and the tail up
    to nbytes.  Fields must be ordered and disjoint (asserted)."""
    out, at = [], 0
    for name, off, size in extents:
        assert off >= at, (name, off, at)
        if off > at:
            out.append((at, off))
        at = off + size
    assert at <= nbytes, (at, nbytes)
    if at < nbytes:
        out.append((at, nbytes))
    return out


def clear_spans(kind, extents):
    """[(lo, hi)]: what the host code clears with one fill ACROSS field boundaries, padding included (csrc/rrl_ws.h: the
    first six fields; MHIST .. MSUM; GACC up to KJC's offset.  The wide workspace: STATUS and NSEL)."""
    off = {name: o for name, o, _ in extents}
    if kind == 1:
        return [(off["status"], off["rec"])]
    return [(off["status"], off["hit1"]), (off["mhist"], off["mcand"]), (off["gacc"], off["kjc"])]


def check_gaps(ws, kind, dims, fill):
    """Every gap byte of workspace tensor `ws` (uint8, the middle of a guarded buffer that was filled with `fill`) still
    holds `fill` -- inside a documented clear span: `fill` or zero.  Returns the number of gap bytes checked."""
    ext = field_extents(kind, *dims)
    spans = clear_spans(kind, ext)
    checked = 0
    for lo, hi in gaps(ext, ws.numel()):
        part = ws[lo:hi]
        ok = part == fill
        if any(a <= lo and hi <= b for a, b in spans):
            ok = ok | (part == 0)
        bad = (~ok).nonzero()
        assert bad.numel() == 0, (f"workspace kind {kind} at {dims}: gap [{lo}, {hi}) was written at byte "
                                  f"{lo + int(bad[0])} (fill 0x{fill:02X}, found 0x{int(part[int(bad[0])]):02X})")
        checked += hi - lo
    return checked


# ---------------------------------------------------------------------------------------------------- inputs
# Small shapes select too few lines as the sampler draws them: L = 129 lines on 70 / 130 triangles of synth.make_pair select
# about 30, and no stream, cloud density or triangle size tried reaches 64 (the most seen: 63).  The line sets of the
# workspace tests are therefore a SUBSET of what the reference's sampler draws, in its order: of 6 L sampled lines the first
# ones are taken so that three quarters of the L kept (or all that were drawn) are selected by the bucket range and the rest is not (lines that
# miss a cloud or hit more than the range takes: those paths stay covered).  Where L sampled lines select 96 or more by
# themselves they are taken as they are.  tests/test_ws_layout_host.py asserts the counts on the CPU.
NARROW = (1, 1, 5, 5)
_samples = {}


def counts_of(oracle, s, rng=NARROW):
    """(selected mask, count1, count2) of sample s = dict(tri1, tri2, lines) from the C oracle's scan."""
    import numpy as np
    s1, s2 = oracle.scan(s["tri1"], s["lines"], cap=8), oracle.scan(s["tri2"], s["lines"], cap=8)
    assert not s1["nan"] and not s2["nan"]
    c1, c2 = np.asarray(s1["count"]), np.asarray(s2["count"])
    return (c1 >= rng[0]) & (c1 < rng[2]) & (c2 >= rng[1]) & (c2 < rng[3]), c1, c2


def sample(oracle, seed, n, m, nl, stream=0, shrink=1.0, rng=NARROW):
    """dict(tri1 (n, 9), tri2 (m, 9), lines (nl, 6)) float32: synth.make_pair(seed, n, m) -- shrink < 1: every triangle moved
    towards the cloud's centre, its size kept (test_gpu_scan_levels' dense clouds: more hits per line) -- with nl lines of
    the reference's sampler, chosen as described above."""
    import numpy as np
    from rrl_hip import synth
    key = (seed, n, m, nl, stream, shrink, tuple(rng))
    if key in _samples:
        return _samples[key]
    p = synth.make_pair(seed, n, m)
    f = np.float32(shrink)
    out = {}
    for cloud, name in (("src", "tri1"), ("tar", "tri2")):
        tri = p[cloud + "_tri"].reshape(-1, 3, 3)
        c = tri.mean(1, keepdims=True)
        out[name] = np.ascontiguousarray((tri - (1.0 - f) * c).reshape(-1, 9), np.float32)
        out[cloud] = (p[cloud] * f).astype(np.float32)
    def draw(k):
        lines = oracle.resample_lines(synth.uniform_streams(stream, 10, k), float(f) * float(p["radius"]),
                                      np.asarray(f * p["center"], np.float32), out["src"], out["tar"], k)
        lines = np.ascontiguousarray(lines, np.float32)
        return lines, counts_of(oracle, dict(out, lines=lines), rng)[0]
    drawn, sel = draw(nl)
    if int(sel.sum()) >= 96:
        keep = np.arange(nl)
    else:
        drawn, sel = draw(6 * nl)
        want_sel = min((3 * nl + 3) // 4, int(sel.sum()))
        yes, no = np.flatnonzero(sel)[:want_sel], np.flatnonzero(~sel)[:nl - want_sel]
        assert want_sel >= 64 and len(no) == nl - want_sel, (key, want_sel, len(no))
        keep = np.sort(np.concatenate([yes, no]))
    out["lines"] = np.ascontiguousarray(drawn[keep])
    _samples[key] = out
    return out


def batch(oracle, B, n, m, nl, seed, stream=0, shrink=1.0, rng=NARROW):
    """B samples (seed + b) stacked: dict(tri1 (B, n, 9), tri2 (B, m, 9), lines (B, nl, 6), samples [...])."""
    import numpy as np
    ss = [sample(oracle, seed + b, n, m, nl, stream, shrink, rng) for b in range(B)]
    return dict(tri1=np.stack([s["tri1"] for s in ss]), tri2=np.stack([s["tri2"] for s in ss]),
                lines=np.stack([s["lines"] for s in ss]), samples=ss)


# The shapes of the route table (tests/test_gpu_workspace.py): name -> (B, N, M, L, shrink, bucket range).  Variant v of a
# shape (v = 1: the "other clouds and lines" of the dirty fills) takes seeds and streams of its own.
SHAPES = {
    "levels": (2, 70, 130, 129, 1.0, NARROW),        # partial supergroup, half and wavefront (test_gpu_scan_levels.py)
    "two_tiles": (3, 512, 512, 1025, 1.0, NARROW),   # two line tiles, the second holds one line
    "wide_sort": (2, 4097, 300, 600, 1.0, NARROW),   # a cloud beyond 4096 triangles: HISTG
    "prepared": (2, 512, 512, 1025, 1.0, NARROW),
    "chain_lean": (2, 1200, 1000, 3100, 1.0, NARROW),  # test_chained_and_fat_launches_at_their_smallest_shapes
    "chain_fat": (2, 1200, 1000, 2500, 1.0, NARROW),
    "registration": (2, 200, 180, 600, 1.0, NARROW),
    "ragged": (3, 130, 130, 257, 1.0, NARROW),       # capacities; RAGGED_COUNTS says what each sample has
}
RAGGED_COUNTS = ((0, 130, 100), (130, 130, 90), (257, 257, 200))  # count1, count2, nlines per sample: empty, full, partial
_SEEDS = {"levels": 1300, "two_tiles": 1310, "wide_sort": 1320, "prepared": 1330, "chain_lean": 1500, "chain_fat": 1500,
          "registration": 1340, "ragged": 1350}
STREAMS = {}  # (shape name, variant) -> stream, where the default (the variant's number) is not taken


def shape_batch(oracle, name, variant=0):
    """The batch of table shape `name` (variant 0: the inputs under test; 1: other clouds and lines of the same shape).  The
    ragged shape: every sample at its own counts, padded to the capacities with NaN rows (never interpreted)."""
    import numpy as np
    B, n, m, nl, shrink, rng = SHAPES[name]
    seed, stream = _SEEDS[name] + 50 * variant, STREAMS.get((name, variant), variant)
    if name != "ragged":
        return dict(batch(oracle, B, n, m, nl, seed, stream, shrink, rng), rng=rng)
    c1, c2, cl = RAGGED_COUNTS
    out = dict(tri1=np.full((B, n, 9), np.nan, np.float32), tri2=np.full((B, m, 9), np.nan, np.float32),
               lines=np.full((B, nl, 6), np.nan, np.float32), samples=[], rng=rng,
               counts1=np.array(c1, np.int32), counts2=np.array(c2, np.int32), nlines=np.array(cl, np.int32))
    for b in range(B):
        if min(c1[b], c2[b], cl[b]) == 0:
            out["samples"].append(None)
            continue
        s = sample(oracle, seed + b, c1[b], c2[b], cl[b], stream, shrink, rng)
        out["tri1"][b, :c1[b]], out["tri2"][b, :c2[b]], out["lines"][b, :cl[b]] = s["tri1"], s["tri2"], s["lines"]
        out["samples"].append(s)
    return out


class _TorchSeam:
    """Stands in for the `torch` module inside rrl_hip.ops: everything is torch's own except the three allocators."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        return self._arena.alloc(size, kw, zero=False)

    def zeros(self, *size, **kw):
        return self._arena.alloc(size, kw, zero=True)

    def empty_like(self, t, **kw):
        if not t.is_cuda or kw:
            return torch.empty_like(t, **kw)
        return self._arena.alloc((tuple(t.shape),), dict(dtype=t.dtype, device=t.device), zero=False)


class Arena:
    """The guarded allocations of one or more evaluations; see the module docstring."""

    device_types = ("cuda",)  # host allocations (pinned read-back buffers) stay torch's own

    def __init__(self, fill, band=BAND):
        self.fill, self.band = int(fill), band
        self.records = []   # [buf, nbytes, middle (uint8)]: every guarded allocation, in order
        self.reuse = {}     # nbytes -> [record]: dirty workspaces / scratches waiting for an allocation of their size
        self.reused = 0

    def alloc(self, size, kw, zero):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        dev = kw.get("device")
        dev = torch.device(dev) if dev is not None else None
        if dev is None or dev.type not in self.device_types or set(kw) - {"dtype", "device"}:
            return (torch.zeros if zero else torch.empty)(*size, **kw)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        numel = 1
        for d in size:
            numel *= int(d)
        nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        if nbytes == 0:
            return (torch.zeros if zero else torch.empty)(*size, **kw)
        pool = self.reuse.get(nbytes)
        if pool and dtype == torch.uint8 and len(size) == 1 and not zero:
            rec = pool.pop(0)
            self.reused += 1
        else:
            buf, mid = guarded(nbytes, self.fill, self.band, dev)
            rec = [buf, nbytes, mid]
            self.records.append(rec)
            if zero:
                mid.zero_()
        return rec[2].view(dtype).reshape(size)

    def recycle(self):
        """The 1-D uint8 allocations made so far (workspaces and scratches) serve the next allocations of their size as
        they are; returns how many wait."""
        self.reuse = {}
        for rec in self.records:
            self.reuse.setdefault(rec[1], []).append(rec)
        return sum(len(v) for v in self.reuse.values())

    def record_of(self, t):
        """The guarded allocation that tensor `t` starts in."""
        p = t.data_ptr()
        for rec in self.records:
            if rec[2].data_ptr() == p:
                return rec
        raise KeyError("tensor is not the start of a guarded allocation")

    def assert_bands(self, what):
        """Both bands of every allocation still hold the fill; returns the number of allocations."""
        for i, (buf, nbytes, _) in enumerate(self.records):
            assert bands_intact(buf, nbytes, self.fill, self.band), \
                f"{what}: a guard band of allocation {i} ({nbytes} bytes, fill 0x{self.fill:02X}) was written"
        return len(self.records)

    @contextlib.contextmanager
    def patch(self, *modules):
        """rrl_hip modules whose `torch` is this arena's seam for the duration of the block."""
        seam = _TorchSeam(self)
        saved = [m.torch for m in modules]
        for m in modules:
            m.torch = seam
        try:
            yield self
        finally:
            for m, t in zip(modules, saved):
                m.torch = t
