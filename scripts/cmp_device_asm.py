"""Compare the device code of two builds, kernel by kernel, without a GPU:

    hipcc <mdfnet_hip/build.py: FLAGS> -S --cuda-device-only -x hip csrc/F.hip -o DIR/F.s     (once per commit, for every file F)
    python scripts/cmp_device_asm.py PARENT_DIR TREE_DIR [F ...]

Per file: the kernel symbols only one side has, and for the common ones whether the instruction sequence (comments dropped, the
function number in local labels dropped: it is the kernel's position in the file) and the resource figures (the .amdhsa_ directives and
the metadata counts: VGPR, AGPR, SGPR, LDS, scratch, spills, and with them the occupancy) are identical.  Prints one markdown table row
per file and the kernels that differ; exit status 1 if anything differs.  With --list F: one row per kernel of file F, both sides."""
import os
import re
import sys

LABEL = re.compile(r"\.L(BB|tmp|func_(?:begin|end))(\d+)")
META = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "max_flat_workgroup_size", "wavefront_size", "kernarg_segment_size")


def kernels(path):
    """name -> (instruction lines, resource lines)"""
    text = open(path).read()
    kern = {m.group(1) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)}
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        name, body = m.group(1), m.group(2)
        if name not in kern:
            continue
        code = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if line:
                code.append(LABEL.sub(r".L\1", line))
        out[name] = [code, []]
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        out[m.group(1)][1] += [l.strip() for l in m.group(2).splitlines()]
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^; Kernel info:\n(.*?)^; COMPUTE_PGM_RSRC2", text, re.M | re.S):      # the compiler's summary: occupancy
        out[m.group(1)][1] += [l.strip() for l in m.group(2).splitlines() if not l.startswith("; codeLenInByte")]
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.M | re.S):
        name = re.search(r"^\s+\.symbol:\s+(\S+)\.kd", m.group(0), re.M).group(1)
        out[name][1] += [l.strip() for l in m.group(0).splitlines() if any("." + k + ":" in l for k in META)]
    return out


def figures(k):
    code, res = k
    get = lambda key: next((l.split(key)[1].split()[0] for l in res if key in l), "?")
    return [str(len(code)), get("; NumVgprs: "), get("; NumAgprs: "), get("; TotalNumSgprs: "), get(".group_segment_fixed_size: "), get("; ScratchSize: "),
            get(".vgpr_spill_count: "), get(".sgpr_spill_count: "), get("; Occupancy: ")]


def listing(a_dir, b_dir, f):
    import subprocess
    a, b = kernels(os.path.join(a_dir, f + ".s")), kernels(os.path.join(b_dir, f + ".s"))
    names = sorted(set(a) | set(b))
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    print("| kernel | side | sequence | instructions | VGPR | AGPR | SGPR | static LDS | scratch B | vspill | sspill | occupancy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for n, d in zip(names, dem):
        d = re.sub(r"\(anonymous namespace\)::|\(.*", "", d).replace("void ", "")
        if n in a:
            print(f"| `{d}` | parent | | " + " | ".join(figures(a[n])) + " |")
        if n in b:
            print(f"| | tree | {'identical' if n in a and a[n] == b[n] else ('differs' if n in a else 'new')} | " + " | ".join(figures(b[n])) + " |")


def main():
    if sys.argv[1] == "--list":
        return listing(*sys.argv[2:5])
    a_dir, b_dir = sys.argv[1:3]
    files = sys.argv[3:] or sorted(f[:-2] for f in os.listdir(a_dir) if f.endswith(".s"))
    bad = 0
    print("| file | kernels parent | kernels tree | only parent | only tree | code identical | resources identical |")
    print("|---|---|---|---|---|---|---|")
    notes = []
    for f in files:
        a, b = kernels(os.path.join(a_dir, f + ".s")), kernels(os.path.join(b_dir, f + ".s"))
        common = sorted(set(a) & set(b))
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        code = [k for k in common if a[k][0] == b[k][0]]
        res = [k for k in common if a[k][1] == b[k][1]]
        print(f"| {f} | {len(a)} | {len(b)} | {len(only_a)} | {len(only_b)} | {len(code)} of {len(common)} | {len(res)} of {len(common)} |")
        notes += [f"{f}: only parent: {k}" for k in only_a] + [f"{f}: only tree: {k}" for k in only_b]
        notes += [f"{f}: differs: {k}" for k in common if a[k] != b[k]]
        bad += len(only_a) + len(only_b) + 2 * len(common) - len(code) - len(res)
    print("\n".join(notes))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
