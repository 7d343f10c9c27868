#!/usr/bin/env python3
"""tools/kernel_isa_diff.py OLD NEW [--rename MAP.json] [--arch gfx950] [-v]

Did a source change alter the code a GPU runs?  No GPU, no torch: OLD and NEW are two built libmms_hip.so (or any
file that carries HIP fat binaries, or two directories of such files, e.g. the build/ object directories).  Every
gfx950 code object is unbundled (clang-offload-bundler), and for every kernel the tool reports
  * on which side it exists,
  * whether its instructions are identical (llvm-objdump -d, addresses stripped, encodings kept; the fill between
    a symbol's last instruction and the next symbol is not part of it),
  * whether its resource metadata is identical (VGPR / AGPR / SGPR counts, LDS, scratch, kernarg size, ... from the
    code object's notes).
Symbols are matched by MANGLED name (shown demangled where a demangler is installed).  MAP.json is a list of
[regex, replacement] pairs applied to OLD's mangled names, for kernels whose template argument list changed, e.g. a
bool parameter dropped from the fourth place where it was false:
  [["(27euclid_rows_wave_f16_kernelILi\\\\d+ELi\\\\d+ELb[01]E)Lb0E", "\\\\1"]]
Device functions that were not inlined are compared the same way (listed as `func`).
Exit status 0: everything present on both sides is identical; 1: something differs."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size", ".vgpr_spill_count",
             ".sgpr_spill_count", ".uses_dynamic_stack")


def tool(name):
    for d in (os.environ.get("LLVM_BIN"), "/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    p = shutil.which(name)
    if not p:
        sys.exit("kernel_isa_diff: %s not found (set LLVM_BIN)" % name)
    return p


def run(*cmd, stdin=None):
    return subprocess.run(cmd, check=True, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE).stdout


def demangle(names):
    """llvm-cxxfilt or binutils' c++filt, whichever exists; without one the mangled names are kept."""
    for d in (os.environ.get("LLVM_BIN"), "/opt/rocm/llvm/bin", None):
        for n in ("llvm-cxxfilt", "c++filt"):
            p = os.path.join(d, n) if d else shutil.which(n)
            if p and os.path.exists(p):
                return run(p, stdin="\n".join(names).encode()).decode().splitlines()
    return list(names)


def code_objects(path, arch, tmp):
    """[(label, code object file)] of every `arch` code object in `path` (a file, or a directory of files)."""
    files = [path] if os.path.isfile(path) else sorted(
        os.path.join(path, f) for f in os.listdir(path) if f.endswith((".o", ".so", ".hipfb", ".co")))
    out = []
    for f in files:
        fat = os.path.join(tmp, "fat%d.bin" % len(os.listdir(tmp)))
        if open(f, "rb").read(len(MAGIC)) == MAGIC:
            shutil.copy(f, fat)
        else:
            subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, f, os.devnull], check=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]   # a linked library: one bundle per source
        for i, s in enumerate(starts):
            piece, co = fat + ".%d" % i, fat + ".%d.co" % i
            open(piece, "wb").write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
            run(tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hip-amdgcn-amd-amdhsa--" + arch,
                "--input=" + piece, "--output=" + co)
            if os.path.getsize(co):
                label = os.path.basename(f) if len(starts) == 1 else "%s[%d]" % (os.path.basename(f), i)
                out.append((label, co))
    return out


def metadata(co):
    """{mangled kernel name: {key: value}} from the amdhsa.kernels note."""
    kernels, cur = {}, None
    for line in run(tool("llvm-readelf"), "--notes", co).decode().splitlines():
        m = re.match(r"^  (- | {2})(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3).strip("'\"")
        if m.group(2) == ".name":
            kernels[cur[".name"]] = cur
    return {k: {key: v.get(key) for key in META_KEYS} for k, v in kernels.items()}


def disassembly(co):
    """{mangled symbol: [instruction lines without addresses; branch targets relative to the symbol, written <@+0x..>]}"""
    syms, cur, own = {}, None, None
    for line in run(tool("llvm-objdump"), "-d", co).decode().splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            own = m.group(1)
            cur = syms.setdefault(own, [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line.strip()).replace("<" + own + "+", "<@+"))
    # What follows a symbol's last instruction is the gap to whatever the linker placed next (zero fill shown as
    # `...`, s_nop 0 or s_code_end fill; the end-of-section pad after the last kernel of a code object): it depends
    # on the symbol's neighbours, so it changes when kernels move between sources, and no wave executes it.
    for isa in syms.values():
        while isa and re.match(r"^(\.\.\.|s_nop 0|s_code_end)(\s|$)", isa[-1]):
            isa.pop()
    return syms


def load(path, arch, renames):
    side = {}
    with tempfile.TemporaryDirectory() as tmp:
        cos = code_objects(path, arch, tmp)
        if not cos:
            sys.exit("kernel_isa_diff: no %s code object in %s" % (arch, path))
        for label, co in cos:
            meta, dis = metadata(co), disassembly(co)
            names = sorted(dis)
            for mangled, plain in zip(names, demangle(names)):
                key = mangled
                for pat, rep in renames:
                    key = re.sub(pat, rep, key)
                while key in side:                     # the same template instance in a second code object
                    key += "'"
                side[key] = {"co": label, "name": plain, "isa": dis[mangled], "meta": meta.get(mangled),
                             "kernel": mangled in meta}
    return side


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", help="JSON list of [regex, replacement] applied to OLD's mangled names")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("-v", "--verbose", action="store_true", help="also list the identical symbols")
    a = ap.parse_args()
    renames = json.load(open(a.rename)) if a.rename else []
    old, new = load(a.old, a.arch, renames), load(a.new, a.arch, [])
    counts = {"identical": 0, "differs": 0, "only old": 0, "only new": 0}
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        kind = "kernel" if (o or n)["kernel"] else "func"
        if o and n:
            isa, meta = o["isa"] == n["isa"], o["meta"] == n["meta"]
            state = "identical" if isa and meta else "differs"
            detail = "isa %s (%d / %d instructions), metadata %s" % (
                "same" if isa else "DIFFERS", len(o["isa"]), len(n["isa"]), "same" if meta else "DIFFERS")
            if not isa:
                first = next((i for i, (x, y) in enumerate(zip(o["isa"], n["isa"])) if x != y), min(len(o["isa"]), len(n["isa"])))
                detail += "\n    first difference at instruction %d:\n      old: %s\n      new: %s" % (
                    first, " ".join((o["isa"][first:first + 1] or ["(end)"])[0].split()),
                    " ".join((n["isa"][first:first + 1] or ["(end)"])[0].split()))
            if not meta:
                detail += " " + ", ".join("%s %s -> %s" % (k, o["meta"][k], n["meta"][k]) for k in META_KEYS
                                          if o["meta"] and n["meta"] and o["meta"][k] != n["meta"][k])
        else:
            state, detail = ("only old" if o else "only new"), ""
        counts[state] += 1
        if a.verbose or state != "identical":
            print("%-9s %-6s %-28s %s  %s" % (state, kind, (o or n)["co"], (n or o)["name"], detail))
    for tag, side in (("old", old), ("new", new)):
        per = {}
        for v in side.values():
            if v["kernel"]:
                per[v["co"]] = per.get(v["co"], 0) + 1
        print("%s: %d kernels: %s" % (tag, sum(per.values()), ", ".join("%s %d" % kv for kv in per.items())))
    print("both sides: %(identical)d identical, %(differs)d differ; only old: %(only old)d; only new: %(only new)d" % counts)
    return 1 if counts["differs"] else 0


if __name__ == "__main__":
    sys.exit(main())
