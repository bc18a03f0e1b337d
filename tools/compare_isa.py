#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two builds, kernel by kernel.

    for f in vae_equalizer_amd/csrc/*.hip; do
        hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -I include -I vae_equalizer_amd/csrc $f -o OUT/$(basename $f).s
    done                                                   # once per build (the form tools/scan_isa.py reads)
    python tools/compare_isa.py OLD_DIR NEW_DIR [--expect-changed SUBSTRING ...]

A kernel is identical when its instructions match one for one after branch labels are renumbered in order of appearance (which translation
unit holds it, and in what order, does not matter).  Kernels whose demangled name contains one of the --expect-changed substrings are
reported with instruction count, VGPRs and LDS of both builds instead.  Exit status 1 if any other kernel differs, appears or disappears.
"""
import glob
import os
import re
import subprocess
import sys


def kernels(directory):
    """{mangled name: (instruction tuple, vgprs, lds bytes)} over every .s file of the directory"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m}
        i = 0
        while i < len(lines):
            m = re.match(r"(\w+):\s*(;.*)?$", lines[i])
            if not (m and m.group(1) in names):
                i += 1
                continue
            name, body, labels = m.group(1), [], {}
            i += 1
            while not lines[i].startswith(".Lfunc_end"):
                ln = lines[i].split(";")[0].strip()
                i += 1
                if not ln or ln.startswith("."):               # labels and directives
                    continue
                ln = re.sub(r"\.LBB\d+_\d+", lambda t: labels.setdefault(t.group(0), "L%d" % len(labels)), ln)
                body.append(re.sub(r"\s+", " ", ln))
            info = {}
            while i < len(lines) and not re.match(r"\s*\.(globl|protected|weak)\s", lines[i]):     # the "; Kernel info:" comments behind the body
                t = re.match(r";\s*(NumVgprs|LDSByteSize):\s*(\d+)", lines[i])
                if t:
                    info[t.group(1)] = int(t.group(2))
                i += 1
            out[name] = (tuple(body), info.get("NumVgprs"), info.get("LDSByteSize"))
        missed = names - set(out)
        if missed:                                             # a body this parser did not find must not read as "identical"
            sys.exit("%s: no body found for %d of %d kernels, e.g. %s" % (path, len(missed), len(names), sorted(missed)[0]))
    return out


def main():
    args = sys.argv[1:]
    expect = []
    if "--expect-changed" in args:
        k = args.index("--expect-changed")
        expect, args = args[k + 1:], args[:k]
    old, new = kernels(args[0]), kernels(args[1])
    names = sorted(set(old) | set(new))
    plain = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    same = bad = 0
    for n in names:
        if any(e in plain[n] for e in expect):
            o, w = old.get(n), new.get(n)
            fmt = lambda k: "absent" if k is None else "%d instructions, %s VGPRs, %s B LDS" % (len(k[0]), k[1], k[2])
            print("moved  %s\n         before: %s\n         after:  %s" % (plain[n], fmt(o), fmt(w)))
        elif n in old and n in new and old[n][0] == new[n][0]:
            same += 1
        else:
            bad += 1
            print("DIFFERS %s (%s -> %s instructions)" % (plain[n], len(old[n][0]) if n in old else "absent", len(new[n][0]) if n in new else "absent"))
    print("%d kernels compared outside the expected set: %d identical, %d different" % (same + bad, same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
