#!/usr/bin/env python3
"""One sha256 per translation unit of the DEVICE assembly of librrl_hip (no GPU needed).

Every file of rrl_hip.build.SOURCES is compiled with build.FLAGS and its per-file extras plus `--cuda-device-only -S`;
the lines that contain `__hip_cuid_` (a symbol that hashes the source path) are dropped and the rest is hashed.  Two
source trees with equal digests launch the same machine code: a host-side change proves that way that no kernel moved.

    python tools/device_asm_digest.py [--csrc DIR] [--json OUT] [--label NAME]

--json merges {NAME: {file: digest}} into OUT (profiles/call_record_device_asm.json holds `parent` and `branch`).
"""
import argparse
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_module():
    path = os.path.join(ROOT, "a-robust-registration-loss_amd", "rrl_hip", "build.py")
    spec = importlib.util.spec_from_file_location("rrl_hip_build", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digest(build, csrc, src, tmp):
    extra = ["-fno-slp-vectorize"] if src == "rrl_cull.hip" else []  # as build.build_lib
    out = os.path.join(tmp, src.replace(".hip", ".s"))
    subprocess.check_call([build._hipcc(), *build.FLAGS, *extra, "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out])
    h = hashlib.sha256()
    with open(out, "rb") as f:
        for line in f:
            if b"__hip_cuid_" not in line:
                h.update(line)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=None, help="source directory (default: the tree's csrc)")
    ap.add_argument("--json", default=None, help="merge the digests into this JSON file under --label")
    ap.add_argument("--label", default="branch")
    ap.add_argument("--jobs", type=int, default=min(9, max(1, (os.cpu_count() or 2) // 2)))
    args = ap.parse_args()
    build = _build_module()
    csrc = os.path.abspath(args.csrc) if args.csrc else build.CSRC
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=args.jobs) as pool:
        sums = dict(zip(build.SOURCES, pool.map(lambda s: digest(build, csrc, s, tmp), build.SOURCES)))
    for src in build.SOURCES:
        print(sums[src], src)
    if args.json:
        doc = {}
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc[args.label] = sums
        if "parent" in doc and "branch" in doc:
            doc["identical"] = doc["parent"] == doc["branch"]
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
