#!/usr/bin/env python3
"""One sha256 per translation unit of the DEVICE assembly of librrl_hip (no GPU needed).

Every file of rrl_hip.build.SOURCES is compiled with build.FLAGS and its per-file extras plus `--cuda-device-only -S`;
the lines that contain `__hip_cuid_` (a symbol that hashes the source path) are dropped and the rest is hashed.  Two
source trees with equal digests launch the same machine code: a host-side change proves that way that no kernel moved.

    python tools/device_asm_digest.py [--csrc DIR] [--json OUT] [--label NAME]

--json merges {NAME: {file: digest}} into OUT (profiles/call_record_device_asm.json holds `parent` and `branch`); units of
the build list that --csrc does not hold are left out (a parent tree against a branch that adds one: `new_units`).

A change that renames kernels moves the whole-file digest although no instruction moved.  For that case

    python tools/device_asm_digest.py --kernels rrl_cull.hip [--csrc DIR] --json OUT --label NAME [--diff TXT]

splits the unit's assembly into its kernels and records, per kernel, one sha256 of the instruction text and one of the
.amdhsa_* block -- the kernel's own symbol replaced by a placeholder, the function number taken out of the local labels
(.LBBn_m, .Lfunc_endn), the .Ltmpn numbered from 0, runs of blanks collapsed -- plus VGPRs (allocated and used), SGPRs, LDS,
scratch, code and kernel-argument bytes.
Once OUT holds `parent` and `branch`, every parent kernel is compared with the branch kernel of the same symbol, or with
the one that OUT's hand-written table "pairs" ([[parent symbol, branch symbol], ...]) names for it; nothing is matched by
resemblance.  --diff writes the normalised diff of the pairs that differ (needs --parent-csrc: the other side is recompiled).
"""
import argparse
import difflib
import hashlib
import importlib.util
import json
import os
import re
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


def assemble(build, csrc, src, tmp):
    extra = ["-fno-slp-vectorize"] if src == "rrl_cull.hip" else []  # as build.build_lib
    out = os.path.join(tmp, src.replace(".hip", ".s"))
    subprocess.check_call([build._hipcc(), *build.FLAGS, *extra, "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out])
    return out


def digest(build, csrc, src, tmp):
    out = assemble(build, csrc, src, tmp)
    h = hashlib.sha256()
    with open(out, "rb") as f:
        for line in f:
            if b"__hip_cuid_" not in line:
                h.update(line)
    return h.hexdigest()


_INFO = {"vgprs_used": "NumVgprs", "sgprs": "TotalNumSgprs", "lds_bytes": "LDSByteSize", "scratch_bytes": "ScratchSize",
         "code_bytes": "codeLenInByte"}


def split_kernels(path):
    """{symbol: {"text": [lines], "amdhsa": [lines], numbers...}} of one device assembly file, normalised (module docstring)."""
    with open(path) as f:
        lines = f.read().split("\n")
    kernels, i = {}, 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        sym, text, hsa, tmps = m.group(1), [], [], {}

        def norm(ln):
            ln = ln.replace(sym, "<kernel>")
            ln = re.sub(r"BB\d+_", "BB_", re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln))  # (.LBBn_m, and BBn_m in loop comments)
            ln = re.sub(r"\.Ltmp\d+", lambda t: ".Ltmp%d" % tmps.setdefault(t.group(0), len(tmps)), ln)
            return re.sub(r"[ \t]+", " ", ln)  # (the comment column moves with the length of a label)

        i += 1
        while not re.match(r"\.Lfunc_end\d+:", lines[i]):
            if lines[i].lstrip().startswith(".amdhsa_kernel"):
                while not lines[i].lstrip().startswith(".end_amdhsa_kernel"):
                    hsa.append(norm(lines[i]))
                    i += 1
            elif lines[i].split()[:1] not in ([".section"], [".text"]):  # (the descriptor sits in .rodata between the code and its end label)
                text.append(norm(lines[i]))
            i += 1
        k = {"text": text, "amdhsa": hsa}
        while not lines[i].lstrip().startswith("; COMPUTE_PGM_RSRC2"):  # the "Kernel info" comment block behind the code
            for key, name in _INFO.items():
                m = re.match(r"; %s\s*[:=]\s*(\d+)" % name, lines[i])
                if m:
                    k[key] = int(m.group(1))
            i += 1
        k["kernarg_bytes"] = next(int(h.split()[-1]) for h in hsa if ".amdhsa_kernarg_size" in h)
        k["vgprs"] = next(int(h.split()[-1]) for h in hsa if ".amdhsa_next_free_vgpr" in h)  # allocated (the waves-per-SIMD budget's)
        kernels[sym] = k
    return kernels


def _sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def kernels_main(args, build, csrc):
    with tempfile.TemporaryDirectory() as tmp:
        mine = split_kernels(assemble(build, csrc, args.kernels, tmp))
        doc = {}
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc[args.label] = {s: dict({x: v for x, v in k.items() if x not in ("text", "amdhsa")}, text=_sha(k["text"]), amdhsa=_sha(k["amdhsa"]))
                           for s, k in mine.items()}
        for s, k in doc[args.label].items():
            print(k["text"][:16], k["amdhsa"][:16], "vgpr %3d sgpr %3d lds %6d scratch %d code %6d" %
                  (k["vgprs"], k["sgprs"], k["lds_bytes"], k["scratch_bytes"], k["code_bytes"]), s[:60])
        differ = []
        if "parent" in doc and "branch" in doc:
            pairs = dict(doc.get("pairs", []))
            doc["verdict"] = {}
            for s, p in doc["parent"].items():
                b = doc["branch"].get(pairs.get(s, s))
                v = "missing" if b is None else "identical" if p == b else "differs: " + ", ".join(x for x in p if p[x] != b.get(x))
                doc["verdict"][s] = v
                if b is not None and p != b:
                    differ.append((s, pairs.get(s, s)))
            doc["identical"] = all(v == "identical" for v in doc["verdict"].values())
            print("identical:", doc["identical"], "--", len(differ), "of", len(doc["parent"]), "kernels differ")
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        if args.diff and differ:
            other = split_kernels(assemble(build, os.path.abspath(args.parent_csrc), args.kernels, os.path.join(tmp, "")))
            old, new = (other, mine) if args.label == "branch" else (mine, other)
            with open(args.diff, "w") as f:
                for p, b in differ:
                    for part in ("text", "amdhsa"):
                        f.writelines(x + "\n" for x in difflib.unified_diff(old[p][part], new[b][part], "parent " + p, "branch " + b, lineterm=""))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=None, help="source directory (default: the tree's csrc)")
    ap.add_argument("--json", default=None, help="merge the digests into this JSON file under --label")
    ap.add_argument("--label", default="branch")
    ap.add_argument("--jobs", type=int, default=min(9, max(1, (os.cpu_count() or 2) // 2)))
    ap.add_argument("--kernels", default=None, metavar="UNIT", help="per-kernel digests of this one unit (needs --json)")
    ap.add_argument("--diff", default=None, help="--kernels: write the normalised diff of the kernels that differ here")
    ap.add_argument("--parent-csrc", default=None, help="--diff: the other tree's source directory")
    args = ap.parse_args()
    build = _build_module()
    csrc = os.path.abspath(args.csrc) if args.csrc else build.CSRC
    if args.kernels:
        return kernels_main(args, build, csrc)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=args.jobs) as pool:
        sources = [s for s in build.SOURCES if os.path.exists(os.path.join(csrc, s))]  # (a parent tree lacks a unit its branch adds)
        sums = dict(zip(sources, pool.map(lambda s: digest(build, csrc, s, tmp), sources)))
    for src in sources:
        print(sums[src], src)
    if args.json:
        doc = {}
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc[args.label] = sums
        if "parent" in doc and "branch" in doc:
            doc["identical"] = all(doc["branch"].get(k) == v for k, v in doc["parent"].items())  # every unit the parent has
            doc["new_units"] = sorted(set(doc["branch"]) - set(doc["parent"]))
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
