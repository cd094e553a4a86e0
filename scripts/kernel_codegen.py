#!/usr/bin/env python3
"""Per-kernel code generation of two builds of one .hip file, side by side: registers, scratch, static LDS, instruction count,
and whether the instruction streams are the same.  For refactors that must not move the kernels.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S -o parent.s rawdtw_runs.hip   (at the parent)
    hipcc ...                                                                   -o new.s    rawdtw_runs.hip   (at the new tree)
    python scripts/kernel_codegen.py parent.s new.s [out.json]
"""
import hashlib
import json
import re
import subprocess
import sys

FIGURES = (("vgpr", r"^; NumVgprs: (\d+)"), ("agpr", r"^; NumAgprs: (\d+)"), ("sgpr", r"^; TotalNumSgprs: (\d+)"),
           ("scratch_bytes", r"^; ScratchSize: (\d+)"), ("lds_bytes", r"^; LDSByteSize: (\d+)"), ("occupancy", r"^; Occupancy: (\d+)"))


def parse(path):
    """{mangled kernel: figures}; a kernel's body runs from its label to .Lfunc_end, its figures follow in comments"""
    out, cur, last, body = {}, None, None, []
    for ln in open(path):
        ln = ln.rstrip("\n")
        if cur is None:
            m = re.match(r"^(_Z\w+):\s*(;.*)?$", ln)
            if m:
                cur, body = m.group(1), []
                continue
            for key, pat in FIGURES:
                m = re.match(pat, ln)
                if m and last:
                    out[last][key] = int(m.group(1))
        elif ln.startswith(".Lfunc_end"):
            out[cur] = {"instructions": len(body), "stream_sha1": hashlib.sha1("\n".join(body).encode()).hexdigest()[:16]}
            cur, last = None, cur
        else:
            s = re.sub(r"\s*;.*$", "", ln.strip())
            if s and not s.startswith(".") and not re.match(r"^[.\w$]+:", s):  # (directives and labels are no instructions)
                body.append(s)
    return out


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(set(a) | set(b))
    plain = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")))
    rows = []
    for k in names:
        name = re.sub(r"\(.*", "", plain[k]).replace("void ", "")
        pa, pb = a.get(k), b.get(k)
        same = bool(pa and pb and pa["stream_sha1"] == pb["stream_sha1"])
        rows.append({"kernel": name, "identical_stream": same, "parent": pa, "new": pb})
        show = lambda p: "-" if not p else "%4d v %3d s %4d scr %6d lds %5d ins" % (p["vgpr"], p["sgpr"], p["scratch_bytes"], p["lds_bytes"], p["instructions"])
        print("%-32s %-9s parent %s | new %s" % (name[:32], "identical" if same else "DIFFERS", show(pa), show(pb)))
    if len(sys.argv) > 3:
        json.dump(rows, open(sys.argv[3], "w"), indent=1)
        print("wrote", sys.argv[3])
    worse = [r["kernel"] for r in rows if r["parent"] and r["new"] and
             any(r["new"][f] > r["parent"][f] for f in ("vgpr", "agpr", "sgpr", "scratch_bytes", "lds_bytes"))]
    if worse:
        sys.exit("registers, scratch or LDS rose: " + ", ".join(worse))


if __name__ == "__main__":
    main()
