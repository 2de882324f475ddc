"""Per-kernel gfx950 ISA comparison of HIP sources between two git revisions, or a revision and the work tree
(dev tool, CPU only): one line per kernel, identical / DIFFERENT, with the compiler's resource figures for both.

    python tools/isa_diff.py s3od_amd/csrc/attention.hip HEAD            # HEAD against the work tree
    python tools/isa_diff.py s3od_amd/csrc/attention.hip HEAD~2 HEAD
    python tools/isa_diff.py s3od_amd/csrc/conv_ops.hip s3od_amd/csrc/linear_ops.hip HEAD     # several sources, one run

The exit status is 1 when any kernel is DIFFERENT or has no partner on the other side; --allow-different makes it 0.
For a DIFFERENT kernel a second line says whether its ordered list of vector-memory instructions (mnemonic, plus the
`lds` modifier), `s_waitcnt vmcnt(N)` values and `s_barrier`s -- what a hand-counted vmcnt relies on -- and its
multiset of opcodes equal the other side's.  With --vmem-order the exit status is 1 only when a kernel has no partner,
a resource figure differs (spill counts and scratch may go down) or that list differs -- compared per basic block,
so that a loop the compiler merely placed elsewhere passes, and not at all for a kernel that spilled to scratch on
the first side, which cannot be counting its vector-memory queue by hand.

Each side's csrc/ is compiled with the flags the Makefile gives that file.  The texts compared are the kernel bodies
without comments, debug and section directives and blank lines, with the kernel's own mangled name and the per-file function
numbers of local labels replaced, and the enclosing function's name dropped from the symbol of a function-local constant
table, which moves when the table moves into a shared helper (its contents are not compared) (a kernel whose function or template parameters changed pairs with its one namesake).
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
KEYS = ["VGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def figures_hold(ra, rb):
    """the resource figures are equal; spill counts and scratch may also have gone down"""
    return all(int(rb.get(k, -1)) <= int(ra.get(k, -1)) if "Spill" in k or "Scratch" in k else ra.get(k) == rb.get(k) for k in KEYS)


def opcodes(body):
    return sorted(l.split()[0] for l in body.splitlines() if l[:1].isspace() and not l.lstrip().startswith("."))


def vmem_order(body, blocks=False):
    """the vector-memory instructions, vmcnt waits and barriers of a kernel body in the order of the text; blocks: one
    such list per basic block, sorted, which does not depend on where the compiler placed the blocks"""
    if blocks:
        return sorted(o for o in (vmem_order(b) for b in re.split(r"(?m)^\.L\w+:|^\s+s_c?branch\w*\s.*$", body)) if o)
    out = []
    for l in body.splitlines():
        op = (l.split() or [""])[0]
        if re.match(r"(buffer|global|flat|scratch)_", op):
            out.append(op + (" lds" if re.search(r"\blds\b", l) else ""))
        elif op == "s_barrier":
            out.append(op)
        elif op == "s_waitcnt" and (m := re.search(r"vmcnt\((\d+)\)", l)) and m.group(1) != "63":     # 63, the counter's maximum: no wait
            out.append(f"vmcnt({m.group(1)})")
    return out


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
            line = re.sub(r"__const\.\w+\.(\w+)", r"__const.\1", line)     # a function-local table is named after its function
            body.append(re.sub(r"\.L(BB|tmp|func_\w+?)\d+", r".L\1", line))
    return out


def diff_source(src, revs, vmem_only=False):
    """prints the report of one source -> the number of kernels that are DIFFERENT (vmem_only: in their vector-memory
    order or resource figures) or unpaired"""
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        a, b = (compile_rev(src, r, tmp) for r in revs)
    print(f"# {src}: {revs[0] or 'work tree'} -> {revs[1] or 'work tree'}")
    # (binutils' c++filt does not know DF16b, __bf16: demangled through the half-precision code in its place)
    dem = lambda n: subprocess.run(["c++filt", n.replace("DF16b", "Dh")], capture_output=True, text=True).stdout.strip()
    short = lambda n: re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", dem(n)).replace("half", "bf16")
    base = lambda n: re.sub(r"<.*$", "", short(n))
    for n in sorted(set(a) - set(b)):     # renamed on the second side: pair with the only unmatched kernel of that name
        cand = [m for m in set(b) - set(a) if short(m) == short(n)] or [m for m in set(b) - set(a) if base(m) == base(n)]
        if len(cand) == 1:
            b[n] = b.pop(cand[0])
    fig = lambda r: " ".join(f"{k.split(' [')[0].replace(' ', '')} {r.get(k, '?')}" for k in KEYS)
    for n in sorted(set(a) | set(b), key=short):
        if n not in a or n not in b:
            print(f"{'only in ' + str(revs[n in b] or 'work tree'):18s} {short(n)}: {fig((a.get(n) or b.get(n))[1])}")
            bad += 1
            continue
        same = a[n][0] == b[n][0]
        print(f"{'identical' if same else 'DIFFERENT':18s} {short(n)}: {fig(a[n][1])}" + ("" if a[n][1] == b[n][1] and same else f" -> {fig(b[n][1])}"))
        if same:
            continue
        order = ("equal" if vmem_order(a[n][0]) == vmem_order(b[n][0]) else
                 "equal per basic block, blocks placed differently" if vmem_order(a[n][0], True) == vmem_order(b[n][0], True) else "DIFFERS")
        ops = opcodes(a[n][0]) == opcodes(b[n][0])
        print(f"{'':18s}   vmem / vmcnt / barrier order {order} ({len(vmem_order(b[n][0]))} entries), opcode multiset "
              f"{'equal' if ops else 'differs'} ({len(opcodes(a[n][0]))} -> {len(opcodes(b[n][0]))} instructions)")
        # a kernel that spills to scratch on the first side does not pace itself by a hand-counted vmcnt: figures only
        counted = a[n][1].get("ScratchSize [bytes/lane]") == "0"
        bad += not ((order != "DIFFERS" or not counted) and figures_hold(a[n][1], b[n][1])) if vmem_only else 1
    return bad


def main():
    args = [a for a in sys.argv[1:] if a not in ("--allow-different", "--vmem-order")]
    srcs = [Path(a) for a in args if a.endswith(".hip")]
    revs = ([a for a in args if not a.endswith(".hip")] + [None])[:2]
    bad = sum([diff_source(src, revs, "--vmem-order" in sys.argv) for src in srcs])
    sys.exit(1 if bad and "--allow-different" not in sys.argv else 0)


if __name__ == "__main__":
    main()
