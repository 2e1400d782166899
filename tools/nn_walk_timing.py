"""Another build of librrl_hip.so (--parent: the parent commit's) against this tree's, both loaded into one process, for the
kernels that csrc/rrl_knn_walk.h and the FPS body template moved: rrl_knn's tree kernels, rrl_knn3_self, rrl_fps and
rrl_fps_counted, at the shapes tools/knn_timing.py and tools/pseudo_triangles_timing.py time.

  method    device events around windows of the same number of calls; the libraries take turns, and the turn order rotates round
            after round.  Every library of a row runs on THE SAME device buffers (inputs, outputs, scratch): two allocations
            of one size at different addresses differ by more than the kernels compared here do.  A row passes when this
            tree's median is at or below the other library's maximum of the same run.  The outputs are compared bit for bit.
  control   --control: a second copy of the parent's library (another file, so the loader maps it again).  The same code
            loaded twice shows what part of a difference is the loading and placement of a library, not its instructions.
  bench     --parent-tree DIR (a checkout of the parent commit with its library built): tools/knn_timing.py's bench_series,
            `python bench.py` alternating between this tree and DIR.
  record    --note TEXT goes into the record's `what`; --superseded WHAT,.. moves the rows of those names under
            `superseded_rows`, out of all_inside_or_below: a measurement of code that was then taken out again stays on record
            as what decided it (profiles/nn_walk_timing.json: --superseded "knn dcp self,knn tree self,knn tree cross").

    python tools/nn_walk_timing.py --parent OTHER/librrl_hip.so [--control COPY.so] [--parent-tree DIR] [--out JSON]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from rrl_hip._abi import PROTOS  # noqa: E402
import knn_timing as KT  # noqa: E402
import pseudo_triangles_timing as PT  # noqa: E402


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in PROTOS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return lib


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / steps


# each maker returns a closure around one entry of `lib` on the buffers in `bufs`, which the first library of a row allocates
# (the parent's: its scratch sizes are the largest) and the others share

def knn_call(lib, bufs, x, k, flags=0, query=None, channels=0):
    B, n = x.shape[:2]
    S = n if query is None else query.shape[1]
    if not bufs:
        C = 3 * bin(channels).count("1")
        bufs.update(idx=torch.empty(B, S, k, dtype=torch.int32, device="cuda"), found=torch.empty(B, S, dtype=torch.int32, device="cuda"),
                    feat=torch.empty(B, max(C, 1), S, k, device="cuda") if channels else None,
                    ws=torch.empty(int(lib.rrl_knn_workspace_bytes(B, n, S)), dtype=torch.uint8, device="cuda"))
    idx, found, feat, ws = bufs["idx"], bufs["found"], bufs["feat"], bufs["ws"]
    assert lib.rrl_knn_workspace_bytes(B, n, S) <= ws.numel()

    def call():
        rc = lib.rrl_knn(P(x), None, P(query), None, k, flags, channels, P(ws), ws.numel(), P(idx), P(found), None, P(feat), B, n, S, stream())
        assert rc == 0, rc
    call.outputs = [idx, found] + ([feat] if channels else [])
    return call


def knn3_call(lib, bufs, x):
    B, n = x.shape[:2]
    if not bufs:
        bufs.update(nn=torch.empty(B, n, 3, dtype=torch.int32, device="cuda"),
                    ws=torch.empty(int(lib.rrl_knn3_self_workspace_bytes(B, n)), dtype=torch.uint8, device="cuda"))
    nn, ws = bufs["nn"], bufs["ws"]
    assert lib.rrl_knn3_self_workspace_bytes(B, n) <= ws.numel()

    def call():
        rc = lib.rrl_knn3_self(P(x), None, P(ws), ws.numel(), P(nn), None, None, B, n, stream())
        assert rc == 0, rc
    call.outputs = [nn]
    return call


def fps_call(lib, bufs, x, S, counted):
    B, n = x.shape[:2]
    if not bufs:
        bufs.update(cnt=torch.full((B,), n, dtype=torch.int32, device="cuda"), st=torch.zeros(B, dtype=torch.int32, device="cuda"),
                    idx=torch.empty(B, S, dtype=torch.int32, device="cuda"), scratch=torch.empty(B, n, dtype=torch.float32, device="cuda"))
    cnt, st, idx, scratch = bufs["cnt"], bufs["st"], bufs["idx"], bufs["scratch"]

    def call():
        if counted:
            rc = lib.rrl_fps_counted(P(x), P(cnt), P(st), P(idx), None, P(scratch), B, n, S, stream())
        else:
            rc = lib.rrl_fps(P(x), P(st), P(idx), P(scratch), B, n, S, stream())
        assert rc == 0, rc
    call.outputs = [idx]
    return call


def compare(what, shape, make, a, rows):
    bufs = {}
    fns = {name: make(lib, bufs) for name, lib in a.libs.items()}
    names = list(fns)
    steps, seen = {}, {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        seen[name] = [o.clone() for o in fn.outputs]
        steps[name] = max(1, min(a.steps, int(a.window_ms * 1e3 / max(timed(fn, 1), 1.0))))
    n = min(steps.values())
    out = {name: [] for name in fns}
    for r in range(a.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            out[name].append(timed(fns[name], n))
    row = dict(what=what, **shape, calls_per_window=n,
               same_bits=all(torch.equal(u, v) for name in names[1:] for u, v in zip(seen["parent"], seen[name])))
    for name, v in out.items():
        row[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    row["inside_or_below"] = row["branch"]["median_us"] <= row["parent"]["max_us"]
    if "control" in row:
        row["control_inside_or_below"] = row["control"]["median_us"] <= row["parent"]["max_us"]
    rows.append(row)
    print(json.dumps(row), flush=True)
    del fns, bufs, seen
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's librrl_hip.so")
    ap.add_argument("--control", help="a second copy of the parent's librrl_hip.so under another file name")
    ap.add_argument("--parent-tree", help="checkout of the parent commit with its library built: adds the bench series")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--note", default="", help="appended to the record's `what`: what was measured, if not the tree as it stands")
    ap.add_argument("--superseded", default="", help="comma-separated `what` of rows that measure code the tree no longer holds: "
                                                      "written under superseded_rows and left out of all_inside_or_below")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_walk_timing.json"))
    a = ap.parse_args()
    from rrl_hip.build import LIB
    a.libs = {"parent": load(os.path.abspath(a.parent))}
    if a.control:
        a.libs["control"] = load(os.path.abspath(a.control))
    a.libs["branch"] = load(LIB)
    rows, doc = [], {}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def save():
        doc.update({"what": "the parent's library%s and this tree's in one process on the same device buffers; windows of about %g ms (the "
                            "same number of calls for each), device events, %d rounds, the turn order rotating; inside_or_below: the median "
                            "<= the parent's maximum" % (", a second copy of it (control)" if a.control else "", a.window_ms, a.rounds),
                    "device": torch.cuda.get_device_name(0), "all_same_bits": all(r["same_bits"] for r in rows)})
        if a.note:
            doc["what"] += ".  " + a.note
        old = [w.strip() for w in a.superseded.split(",") if w.strip()]
        doc["rows"] = [r for r in rows if r["what"] not in old]
        doc["all_inside_or_below"] = all(r["inside_or_below"] for r in doc["rows"])
        if old:
            doc["superseded_rows"] = [r for r in rows if r["what"] in old]
            doc["superseded_rows_outside"] = sum(not r["inside_or_below"] for r in doc["superseded_rows"])
        if a.control:
            doc["control_rows_outside"] = sum(not r["control_inside_or_below"] for r in rows)  # (of all rows, superseded included)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    # tools/knn_timing.py (a): DCP's self form at k = 20 with its features
    for n in (1024, 2048):
        x = KT.cloud("surface", 500 + n, 8, n)
        compare("knn dcp self", dict(B=8, n=n, k=20, channels=5), lambda lib, bufs: knn_call(lib, bufs, x, 20, 2, channels=5), a, rows)
    save()
    # (b): the tree part, self form
    for n in (1024, 4096, 16384, 65536, 262144):
        for B in (1, 8):
            for kind in KT.KINDS:
                x = KT.cloud(kind, 70 + n, B, n)
                for k in (20, 3):
                    compare("knn tree self", dict(B=B, n=n, k=k, kind=kind), lambda lib, bufs: knn_call(lib, bufs, x, k), a, rows)
                del x
        save()
    x = KT.cloud("surface", 70 + 4096, 8, 4096)
    for k in (8, 16, 32):  # the other unrolled instantiations
        compare("knn tree self", dict(B=8, n=4096, k=k, kind="surface"), lambda lib, bufs: knn_call(lib, bufs, x, k), a, rows)
    # (c): the cross part
    for n in (1024, 4096, 16384):
        x, q = KT.cloud("surface", 900 + n, 8, n), KT.cloud("volume", 901 + n, 8, n) * 0.8
        compare("knn tree cross", dict(B=8, n=n, S=n, k=20), lambda lib, bufs: knn_call(lib, bufs, x, 20, 0, query=q), a, rows)
    save()
    # tools/pseudo_triangles_timing.py: the all-points 3-NN
    for B, sizes in ((1, PT.SIZES_B1 + [PT.TREE_ONLY]), (8, PT.SIZES_B8)):
        for n in sizes:
            for kind in PT.KINDS:
                x = torch.from_numpy(PT.cloud(kind, 7 * n + B, B, n)).cuda()
                compare("knn3_self", dict(B=B, n=n, kind=kind), lambda lib, bufs: knn3_call(lib, bufs, x), a, rows)
                del x
    save()
    # ... and farthest-point sampling, S = 256: in LDS (n = 1024, 4096) and in global scratch (n = 16384), both kernels
    for n in (1024, 4096, 16384):
        x = torch.from_numpy(PT.cloud("surface", 99 + n, 8, n)).cuda()
        for counted in (True, False):
            compare("fps_counted" if counted else "fps", dict(B=8, n=n, S=PT.FPS_S),
                    lambda lib, bufs: fps_call(lib, bufs, x, PT.FPS_S, counted), a, rows)
    save()
    torch.cuda.synchronize()
    if a.parent_tree:
        doc["bench"] = KT.bench_series(os.path.abspath(a.parent_tree), a.bench_rounds)
        save()
    print(json.dumps({k: v for k, v in doc.items() if k not in ("rows", "superseded_rows")}))
    print(json.dumps({"outside": [r for r in rows if not r["inside_or_below"]]}))


if __name__ == "__main__":
    main()
