#!/usr/bin/env python3
"""Per-kernel comparison of two `hipcc --cuda-device-only -S` outputs of the same source file (parent / result): the resource
metadata of each kernel ('; Kernel info:' block) and the number of instructions per mnemonic class.  Nothing is run.
usage: tools/isa_compare.py [--rename-parent REGEX REPLACEMENT] parent.s result.s [label]
(label: the source file's name for the `file` column; --rename-parent: re.sub on the parent's kernel names before the two files are
matched by name, for a kernel whose template parameters changed)
A file that defines no kernel gives an empty table (c++filt is not started without names: it would wait on standard input)."""
import re, subprocess, sys

CLASSES = ("v_mfma", "v_exp_f32", "ds_", "global_", "s_barrier")
META = {"TotalNumSgprs": "sgpr", "NumVgprs": "vgpr", "ScratchSize": "scr", "Occupancy": "occ", "LDSByteSize": "lds", "SGPRBlocks": "sgprblk"}


def kernels(path):
    """{demangled name: {"text": [instruction lines], metadata...}} for every kernel of the file"""
    out, name, body = {}, None, []
    lines = open(path).read().splitlines()
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"^(\w+):\s+; @", ln)
        if m:
            name, body = m.group(1), []
        elif name and ln.startswith(".Lfunc_end"):
            k = {"text": body}
            while i < len(lines) and not lines[i].startswith("; Occupancy"):
                m = re.match(r"^; (\w+): (\d+)", lines[i])
                if m and m.group(1) in META:
                    k[META[m.group(1)]] = int(m.group(2))
                i += 1
            k["occ"] = int(lines[i].split(":")[1])
            if ".amdhsa_kernel " + name in "\n".join(lines):     # device functions have no descriptor
                out[name] = k
            name = None
        elif name:
            s = ln.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", s))
        i += 1
    names = subprocess.run(["c++filt"] + list(out), capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout.split("\n") if out else []
    short = lambda n: re.sub(r"^void |\(.*$|pgk::", "", n).replace("__hip_bfloat16", "bf16").replace("_Float16", "f16")
    return {short(n): k for n, k in zip(names, out.values())}


def count(k, cls):
    return sum(1 for s in k["text"] if s.startswith(cls))


def main():
    argv, rename = sys.argv[1:], None
    if argv and argv[0] == "--rename-parent":
        rename, argv = argv[1:3], argv[3:]
    par, res = kernels(argv[0]), kernels(argv[1])
    if rename:
        par = {re.sub(rename[0], rename[1], n): k for n, k in par.items()}
    label = argv[2] if len(argv) > 2 else ""
    print(f"{'kernel (result)':<46s} {'file':<18s} {'VGPR p/r':>9s} {'SGPR p/r':>9s} {'SGPRalloc p/r':>13s} {'occ p/r':>7s} {'LDS p/r':>13s} {'scr p/r':>7s} "
          f"{'mfma p/r':>9s} {'exp p/r':>8s} {'ds p/r':>8s} {'global p/r':>10s} {'barrier p/r':>11s} {'insts p/r':>11s} {'delta':>7s}  verdict")
    for name in sorted(res):
        r, p = res[name], par.get(name)
        if p is None:
            print(f"{name:<46s} {label:<18s} not in the parent")
            continue
        pair = lambda key: f"{p[key]}/{r[key]}"
        cnt = [(count(p, c), count(r, c)) for c in CLASSES]
        np_, nr = len(p["text"]), len(r["text"])
        delta = 100.0 * (nr - np_) / np_
        if p["text"] == r["text"]:
            verdict = "identical"
        else:
            miss = [key for key in ("scr", "occ", "lds", "sgprblk") if p[key] != r[key]] + [c for c, (a, b) in zip(CLASSES, cnt) if a != b]
            if r["scr"] or abs(delta) > 1.0:
                miss.append("insts" if abs(delta) > 1.0 else "scratch")
            verdict = "RULE MISSED: " + ", ".join(miss) if miss else "rule met" + ("" if p["vgpr"] == r["vgpr"] else f", VGPRs {r['vgpr'] - p['vgpr']:+d}")
        cols = [pair("vgpr"), pair("sgpr"), "%d/%d" % ((p["sgprblk"] + 1) * 8, (r["sgprblk"] + 1) * 8), pair("occ"), pair("lds"), pair("scr")]
        cols += ["%d/%d" % c for c in cnt] + ["%d/%d" % (np_, nr)]
        print(f"{name:<46s} {label:<18s} " + " ".join(c.rjust(w) for c, w in zip(cols, (9, 9, 13, 7, 13, 7, 9, 8, 8, 10, 11, 11)))
              + f" {delta:+6.2f}%  {verdict}")
    for name in sorted(set(par) - set(res)):
        print(f"{name:<46s} {label:<18s} only in the parent")


if __name__ == "__main__":
    main()
