r"""python tools/devcode_diff.py OLD.so NEW.so [--map 'REGEX=>REPLACEMENT' ...] -- the gfx950 device code of two builds
of a backend library, kernel by kernel: the proof that a host-side change (how the launchers pick kernels) left every
kernel as it was.  Prints the kernels only one side has and every function of both whose disassembly or
`llvm-readelf --notes` metadata differs (comments, the PC-relative s_add_u32 immediate after an s_getpc_b64 and trailing
padding ignored: the .text layout may move).  Exit status 1 if a function differs or NEW has a kernel OLD has not.

--map renames OLD's functions before the comparison (re.sub on the demangled name, e.g.
'exact_scan_kernel<(-?\d+)>\(ExArgs\)=>exact_scan_kernel<\1, 0>(ExArgs, ExValidArgs, unsigned int const*)'), so that a kernel is compared
with its successor.  A renamed kernel's argument list may have changed shape: for such a pair the immediate offsets of
scalar loads (where the kernel arguments are read) and the metadata lines that carry the name, the arguments and
`.kernarg_segment_size` are left out of the comparison; everything else counts."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin/"


def run(*cmd):
    return subprocess.run([LLVM + cmd[0], *cmd[1:]], check=True, capture_output=True, text=True).stdout


def describe(so, tmp):
    """kernel names, {function: instructions}, {kernel: metadata text} of the library's gfx950 code object"""
    fat, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
    run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so, os.path.join(tmp, "discard.so"))
    run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
        "--input=" + fat, "--output=" + co)
    kernels = {f[7] for f in map(str.split, run("llvm-readelf", "-s", "-W", co).splitlines())
               if len(f) == 8 and f[3:5] == ["FUNC", "GLOBAL"]}
    code, name, prev = {}, None, ""
    for line in run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            name = m.group(1)
            code[name] = []
        elif name and line.strip():
            ins = line.split("//")[0].strip()
            if prev.startswith("s_getpc_b64"):
                ins = re.sub(r"^(s_add_u32 \S+ \S+) \S+$", r"\1 <pc-rel>", ins)
            code[name].append(ins)
            prev = ins
    for ins in code.values():  # the padding up to the next function's alignment is layout too
        while ins and ins[-1] in ("s_nop 0", "..."):
            ins.pop()
    meta, cur = {}, []
    for line in run("llvm-readelf", "--notes", co).splitlines() + ["  - ."]:
        if line.startswith("  - .") or line.startswith("amdhsa.target"):
            names = [l.split()[1] for l in cur if l.startswith("    .name:")]
            if names:
                meta[names[0]] = "\n".join(cur)
            cur = []
        cur.append(line)
    # mangled -> demangled, from the symbol table read twice
    pretty = {a.split()[7]: b.split(None, 7)[7] for a, b in zip(run("llvm-readelf", "-s", "-W", co).splitlines(),
                                                                run("llvm-readelf", "-s", "-W", "--demangle", co).splitlines())
              if len(a.split()) == 8}
    pretty = {f: pretty.get(f, f) for f in kernels | set(code) | set(meta)}
    return ({pretty[k] for k in kernels}, {pretty[f]: c for f, c in code.items()}, {pretty[k]: m for k, m in meta.items()})


def loose(ins, meta):
    """a renamed kernel without what follows its argument list"""
    ins = [re.sub(r"^(s_load_\S+ .*) \S+$", r"\1 <offset>", i) for i in ins]
    keep, skip = [], False
    for line in (meta or "").splitlines():
        if line.startswith("    .args:"):
            skip = True
        elif skip and re.match(r"^    \.", line):
            skip = False
        if not skip and not re.match(r"^    \.(name|symbol|kernarg_segment_size):", line):
            keep.append(line)
    return ins, keep


def main(old, new, maps=()):
    with tempfile.TemporaryDirectory() as tmp:
        (ko, co, mo), (kn, cn, mn) = describe(old, tmp), describe(new, tmp)
    renamed = set()
    for rule in maps:
        pat, repl = rule.split("=>", 1)
        to = {f: re.sub(pat, repl, f) for f in set(ko) | set(co) | set(mo)}
        renamed |= {t for f, t in to.items() if t != f}
        ko = {to[f] for f in ko}
        co, mo = {to[f]: c for f, c in co.items()}, {to[f]: m for f, m in mo.items()}
    for f in renamed & set(co) & set(cn):
        (co[f], mo[f]), (cn[f], mn[f]) = loose(co[f], mo.get(f)), loose(cn[f], mn.get(f))
    print("kernels: %d -> %d; only in OLD: %d; only in NEW: %d" % (len(ko), len(kn), len(ko - kn), len(kn - ko)))
    for k in sorted(kn - ko):
        print("  added:", k)
    bad = [f for f in sorted(set(co) & set(cn)) if co[f] != cn[f] or mo.get(f) != mn.get(f)]
    for f in bad:
        print("  differs:", f, "(code)" if co[f] != cn[f] else "(metadata)")
    print("functions compared: %d (renamed: %d), differing: %d" % (len(set(co) & set(cn)), len(renamed & set(co) & set(cn)), len(bad)))
    return 1 if bad or kn - ko else 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    maps = [argv[i + 1] for i, a in enumerate(argv) if a == "--map"]
    files = [a for i, a in enumerate(argv) if a != "--map" and (i == 0 or argv[i - 1] != "--map")]
    sys.exit(main(files[0], files[1], maps))
