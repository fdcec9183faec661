"""Compare the kernels of two device assembly files (hipcc --cuda-device-only -S of csrc/zbot_sim.hip with
the product build flags, e.g. the parent commit's and this tree's): per kernel symbol the instruction
count and how many instructions differ after renumbering the block labels, plus the resource lines.

    python scripts/kernel_identity.py parent.s new.s > profiles/<name>/kernel_resources.txt
"""
import re
import subprocess
import sys

RES = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    """{symbol: ([instruction lines, labels renumbered in order of appearance], {resource: value})}"""
    text = open(path).read()
    amdhsa = {m.group(1) for m in re.finditer(r"\.amdhsa_kernel (\S+)", text)}
    out, cur, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(\S+):\s*(;.*)?$", line)
        if m and m.group(1) in amdhsa:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            labels = {}
            for l in body:
                lm = re.match(r"^(\.LBB\S+):", l)
                if lm:
                    labels[lm.group(1)] = f"L{len(labels)}"
            ins = []
            for l in body:
                l = l.split(";")[0].rstrip()
                if not l or l.lstrip().startswith("."):
                    if re.match(r"^\.LBB\S+:", l):
                        ins.append(labels[l[:-1]] + ":")
                    continue
                ins.append(re.sub(r"\.LBB[0-9_]+", lambda k: labels.get(k.group(0), k.group(0)), l.strip()))
            out[cur] = [ins, {}]
            cur = None
            continue
        body.append(line)
    # resources from the metadata notes
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if name in out:
            out[name][1] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in RES if re.search(rf"\.{k}:\s+(\d+)", blk)}
    return out


def demangle(names):
    import shutil
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n[:56] for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    short = [re.sub(r"\(.*", "", l.replace("(anonymous namespace)::", "").replace("void ", "")) for l in r.stdout.splitlines()]
    return dict(zip(names, short))


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = demangle(sorted(set(a) | set(b)))
    same = changed = 0
    print(f"{'kernel':56s} {'parent':>7s} {'new':>7s} {'differ':>7s}  resources (new): regs agpr sgpr scratch lds")
    for sym in sorted(names, key=lambda s: names[s]):
        ia, ib = a.get(sym), b.get(sym)
        res = " ".join(str(ib[1].get(k, "-")) for k in RES) if ib else ""
        if ia is None:
            print(f"{names[sym]:56s} {'-':>7s} {len(ib[0]):7d} {'new':>7s}  {res}")
            continue
        if ib is None:
            print(f"{names[sym]:56s} {len(ia[0]):7d} {'-':>7s} {'gone':>7s}")
            changed += 1
            continue
        n = sum(x != y for x, y in zip(ia[0], ib[0])) + abs(len(ia[0]) - len(ib[0]))
        eq = n == 0 and ia[1] == ib[1]
        same += eq
        changed += not eq
        print(f"{names[sym]:56s} {len(ia[0]):7d} {len(ib[0]):7d} {n:7d}  {res}{'' if ia[1] == ib[1] else '  (parent: ' + str(ia[1]) + ')'}")
    print(f"\n{same} kernel symbol(s) of the parent instruction-identical with equal resources, {changed} changed or gone")


if __name__ == "__main__":
    main()
