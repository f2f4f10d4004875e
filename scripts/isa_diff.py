"""Did a source change alter the code of a kernel?  Compare the gfx950 assembly of one source file in two trees, kernel by kernel.

    python scripts/isa_diff.py TREE_A TREE_B FILE.hip [extra hipcc flags, e.g. -DD4GS_VARIANTS]

Each tree's deblur4dgs_amd/csrc/FILE.hip is compiled device-only with the product's flags (FLAGS, FILE_FLAGS and the fixed -cuid of
this tree's deblur4dgs_amd/build.py) plus the extra ones.  The listing is split per kernel; comments, labels and assembler
directives are dropped; and for every kernel the script prints either "identical" or both sides' instruction count, VGPRs, AGPRs,
SGPRs, LDS bytes, scratch bytes and occupancy.  Exit status 1 if any kernel differs or exists on one side only.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deblur4dgs_amd.build import FILE_FLAGS, FLAGS, _cuid  # noqa: E402

RESOURCES = (("VGPRs", r"\.vgpr_count:\s*(\d+)"), ("AGPRs", r"\.agpr_count:\s*(\d+)"), ("SGPRs", r"\.sgpr_count:\s*(\d+)"),
             ("LDS", r"\.group_segment_fixed_size:\s*(\d+)"), ("scratch", r"\.private_segment_fixed_size:\s*(\d+)"))


def assembly(tree, src, extra):
    with tempfile.TemporaryDirectory() as d:  # (a failing hipcc removes its output file: the directory is what gets cleaned up)
        out = os.path.join(d, "kernels.s")
        cmd = ["hipcc", *FLAGS, *FILE_FLAGS.get(src, []), _cuid(src), *extra, "-S", "--cuda-device-only",
               os.path.join(tree, "deblur4dgs_amd", "csrc", src), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"hipcc failed for {src} of {tree}:\n{r.stderr}")
        return open(out).read()


def kernels(text):
    """name -> {"code": [instruction lines], "Occupancy": n, "VGPRs": n, ...} of every kernel (.amdhsa_kernel) of a listing"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out = {n: {"code": []} for n in names}
    cur, body = None, False  # the kernel a line belongs to; inside its instructions (its resource comments follow the end label)
    for ln in text.splitlines():
        m = re.match(r"^(\S+):\s*(;.*)?$", ln)
        if m and m.group(1) in names:
            cur, body = m.group(1), True
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            body = False
            continue
        m = re.match(r"^; Occupancy:\s*(\d+)", ln)
        if m:
            out[cur]["Occupancy"] = int(m.group(1))
        if not body:
            continue
        code = ln.split(";", 1)[0].strip()
        if code and not code.startswith("."):  # no comments, no directives, no local labels
            out[cur]["code"].append(re.sub(r"\.LBB\d+_", ".LBB_", code))  # (block labels carry the function's number in the file)
    # register / LDS / scratch figures: the kernels' metadata at the end of the listing
    for block in re.split(r"^\s*- \.agpr_count:", text, flags=re.M)[1:]:
        block = "    .agpr_count:" + block
        m = re.search(r"\.name:\s*(\S+)", block)
        if not m or m.group(1) not in out:
            continue
        for key, pat in RESOURCES:
            v = re.search(pat, block)
            out[m.group(1)][key] = int(v.group(1)) if v else None
    return out


def demangled(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    short = r.stdout.splitlines() if r.returncode == 0 else names
    return dict(zip(names, (re.sub(r"^void \(anonymous namespace\)::|\(.*$", "", s) for s in short)))


def main():
    if len(sys.argv) < 4:
        raise SystemExit(__doc__)
    tree_a, tree_b, src, extra = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:]
    a, b = kernels(assembly(tree_a, src, extra)), kernels(assembly(tree_b, src, extra))
    names = sorted(set(a) | set(b))
    pretty = demangled(names)
    print(f"== {src} {' '.join(extra)}".rstrip())
    differ = 0
    for n in names:
        if n not in a or n not in b:
            differ += 1
            print(f"ONLY IN {'A' if n in a else 'B'}  {pretty[n]}")
        elif a[n]["code"] == b[n]["code"]:
            print(f"identical  {pretty[n]}")
        else:
            differ += 1
            fig = lambda k: " ".join([f"instructions {len(k['code'])}"] + [f"{key} {k.get(key)}" for key, _ in RESOURCES] + [f"occupancy {k.get('Occupancy')}"])
            print(f"DIFFERS    {pretty[n]}\n    A: {fig(a[n])}\n    B: {fig(b[n])}")
    print(f"{len(names)} kernels, {'every one identical' if not differ else f'{differ} differ'}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
