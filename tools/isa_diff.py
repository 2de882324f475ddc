"""Per-kernel gfx950 ISA comparison of HIP sources between two git revisions, or a revision and the work tree
(dev tool, CPU only): one line per kernel, identical / DIFFERENT, with the compiler's resource figures for both.

    python tools/isa_diff.py s3od_amd/csrc/attention.hip HEAD            # HEAD against the work tree
    python tools/isa_diff.py s3od_amd/csrc/attention.hip HEAD~2 HEAD
    python tools/isa_diff.py s3od_amd/csrc/conv_ops.hip s3od_amd/csrc/linear_ops.hip HEAD     # several sources, one run

The exit status is 1 when any kernel is DIFFERENT or has no partner on the other side; --allow-different makes it 0.

Each side's csrc/ is compiled with the flags the Makefile gives that file.  The texts compared are the kernel bodies
without comments, debug and section directives and blank lines, with the kernel's own mangled name and the per-file function
numbers of local labels replaced (a kernel whose template parameters went away pairs with its one namesake).
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
KEYS = ["VGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def compile_rev(src, rev, tmp):
    """-> {mangled kernel name: (normalised body, {resource key: value})} of `src` at `rev` (None: the work tree)"""
    d, asm = ROOT / src.parent, Path(tmp) / f"{len(list(Path(tmp).iterdir()))}.s"
    if rev is not None:
        d = Path(tempfile.mkdtemp(dir=tmp))
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, str(src.parent)], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", str(d)], input=tar, check=True)
        d = d / src.parent
    obj = f"build/{src.stem}.o"
    make = subprocess.run(["make", "-C", str(ROOT), "-n", "-B", obj], check=True, capture_output=True, text=True).stdout
    cmd = next(l for l in make.splitlines() if f" -o {obj}" in l).split()
    cmd = [a for a in cmd[:cmd.index("-c")]] + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                               str(d / src.name), "-o", str(asm)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-3000:])
    res, cur = {}, None
    for m in re.finditer(r"remark: +([^:\n]+): *(\S+)", r.stderr):
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    out, name, body = {}, None, []
    for line in asm.read_text().splitlines():
        line = line.split(";", 1)[0].rstrip()
        if not line or re.match(r"\s*\.(file|loc|ident|section|text)\b", line):     # (a template lives in a comdat section)
            continue
        if name is None and line.rstrip(":") in res and line.endswith(":"):
            name, body = line[:-1], []
        elif name is not None and line.startswith(".Lfunc_end"):
            out[name] = ("\n".join(body).replace(name, "KERNEL"), res[name])
            name = None
        elif name is not None:
            body.append(re.sub(r"\.L(BB|tmp|func_\w+?)\d+", r".L\1", line))
    return out


def diff_source(src, revs):
    """prints the report of one source -> the number of kernels that are DIFFERENT or unpaired"""
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        a, b = (compile_rev(src, r, tmp) for r in revs)
    print(f"# {src}: {revs[0] or 'work tree'} -> {revs[1] or 'work tree'}")
    # (binutils' c++filt does not know DF16b, __bf16: demangled through the half-precision code in its place)
    dem = lambda n: subprocess.run(["c++filt", n.replace("DF16b", "Dh")], capture_output=True, text=True).stdout.strip()
    short = lambda n: re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", dem(n)).replace("half", "bf16")
    base = lambda n: re.sub(r"<.*$", "", short(n))
    for n in sorted(set(a) - set(b)):     # renamed on the second side: pair with the only unmatched kernel of that name
        cand = [m for m in set(b) - set(a) if base(m) == base(n)]
        if len(cand) == 1:
            b[n] = b.pop(cand[0])
    fig = lambda r: " ".join(f"{k.split(' [')[0].replace(' ', '')} {r.get(k, '?')}" for k in KEYS)
    for n in sorted(set(a) | set(b), key=short):
        if n not in a or n not in b:
            print(f"{'only in ' + str(revs[n in b] or 'work tree'):18s} {short(n)}: {fig((a.get(n) or b.get(n))[1])}")
            bad += 1
            continue
        same = a[n][0] == b[n][0]
        bad += not same
        print(f"{'identical' if same else 'DIFFERENT':18s} {short(n)}: {fig(a[n][1])}" + ("" if a[n][1] == b[n][1] and same else f" -> {fig(b[n][1])}"))
    return bad


def main():
    args = [a for a in sys.argv[1:] if a != "--allow-different"]
    srcs = [Path(a) for a in args if a.endswith(".hip")]
    revs = ([a for a in args if not a.endswith(".hip")] + [None])[:2]
    bad = sum([diff_source(src, revs) for src in srcs])
    sys.exit(1 if bad and "--allow-different" not in sys.argv else 0)


if __name__ == "__main__":
    main()
