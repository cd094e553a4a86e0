#!/usr/bin/env python3
"""Per-kernel code generation of two builds of one .hip file, side by side: registers, scratch, static LDS, instruction count,
and whether the instruction streams are the same.  For refactors that must not move the kernels.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S -o parent.s rawdtw_runs.hip   (at the parent)
    hipcc ...                                                                   -o new.s    rawdtw_runs.hip   (at the new tree)
    python scripts/kernel_codegen.py parent.s new.s [out.json [only]]
`only`: a regular expression; kernels whose name it does not match (a library's instantiations, say) are compared all the same and
reported as one row, with their number and whether every one of them has the parent's stream and figures.
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
                # (a local label carries its function's number in the module, which moves with the order of instantiation: .LBB573_2)
                body.append(re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", s))
    return out


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(set(a) | set(b))
    plain = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")))
    only = re.compile(sys.argv[4]) if len(sys.argv) > 4 else None
    rows, rest = [], {"kernel": "(every other kernel)", "count": 0, "identical_stream": True, "same_figures": True}
    for k in names:
        name = re.sub(r"\(.*", "", plain[k].replace("(anonymous namespace)::", "")).replace("void ", "")
        pa, pb = a.get(k), b.get(k)
        same = bool(pa and pb and pa["stream_sha1"] == pb["stream_sha1"])
        if only and not only.search(name):
            rest["count"] += 1
            rest["identical_stream"] &= same
            rest["same_figures"] &= bool(pa and pb and all(pa.get(f) == pb.get(f) for f, _ in FIGURES))
            if same:
                continue  # (one that differs gets its own row)
        rows.append({"kernel": name, "identical_stream": same, "parent": pa, "new": pb})
        show = lambda p: "-" if not p else "%4d v %3d s %4d scr %6d lds %5d ins" % (p["vgpr"], p["sgpr"], p["scratch_bytes"], p["lds_bytes"], p["instructions"])
        print("%-32s %-9s parent %s | new %s" % (name[:32], "identical" if same else "DIFFERS", show(pa), show(pb)))
    if only:
        print("%d other kernels: %s" % (rest["count"], "all identical" if rest["identical_stream"] and rest["same_figures"] else "NOT all identical"))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:  # (a row a line)
            f.write("[\n" + ",\n".join(json.dumps(r) for r in rows + ([rest] if only else [])) + "\n]\n")
        print("wrote", sys.argv[3])
    worse = [r["kernel"] for r in rows if r["parent"] and r["new"] and
             any(r["new"][f] > r["parent"][f] for f in ("vgpr", "agpr", "sgpr", "scratch_bytes", "lds_bytes"))]
    if worse:
        sys.exit("registers, scratch or LDS rose: " + ", ".join(worse))


if __name__ == "__main__":
    main()
