#!/usr/bin/env python3
"""Device-code identity of two builds of the library: disassembles every gfx950 code object of both (as disasm_kernel.py does) and compares
the instruction text per demangled kernel name, addresses and absolute branch targets stripped.  Prints the kernels that differ, were
added or were removed; exit status 1 if a kernel present in both differs.  A kernel that changed its NAME between the builds (it became a
template, say) is compared as a pair with --rename 'OLD NAME=NEW NAME' (demangled, as printed under removed / added; repeatable), or with
--rename-file FILE holding one such pair per line.
--opcodes: under each kernel that differs, the opcodes whose counts changed (old -> new; DPP forms counted apart, as opcode_dpp).
   python tools/_prof/diff_kernels.py old/libmpcg_hip.so new/libmpcg_hip.so [--opcodes] [--rename 'old=new' ...] [--rename-file pairs.txt]"""
import collections, os, re, shutil, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    """{demangled name: [instruction text]} over every code object of `lib`"""
    tmp = tempfile.mkdtemp(prefix="dis_")
    try:
        so = os.path.join(tmp, "lib.so"); shutil.copy(lib, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=tmp)
        text = ""
        for co in sorted(f for f in os.listdir(tmp) if "amdgcn" in f):
            text += "\n" + subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--demangle", os.path.join(tmp, co)], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for fn in re.split(r"\n(?=[0-9a-f]+ <)", text):
        head, _, body = fn.partition("\n")
        m = re.match(r"[0-9a-f]+ <(.*)>:$", head)
        if not m:
            continue
        ins = []
        for l in body.split("\n"):
            l = re.sub(r"\s*//.*$", "", l).strip()                # the trailing address comment
            l = re.sub(r"\s*<[^<>]*\+0x[0-9a-f]+>$", "", l)      # the absolute target objdump appends to a branch
            if l and l != "..." and "file format" not in l and not l.startswith("Disassembly of section"):
                ins.append(l)
        # padding behind the last instruction: how much depends on what follows in the section (a zero dword disassembles as the v_cndmask below)
        while ins and ins[-1] in ("s_nop 0", "s_code_end", "v_cndmask_b32_e32 v0, s0, v0, vcc"):
            ins.pop()
        assert m.group(1) not in out, "two code objects define " + m.group(1)
        out[m.group(1)] = ins
    return out


def opcodes(ins):
    return collections.Counter(l.split()[0] + ("_dpp" if re.search(r"quad_perm|row_|wave_", l) and not l.split()[0].endswith("_dpp") else "") for l in ins if not l.endswith(":"))


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
pairs = []
for i, a in enumerate(sys.argv):
    if a == "--rename":
        pairs.append(sys.argv[i + 1])
    if a == "--rename-file":                                      # one OLD NAME=NEW NAME per line
        pairs += [l.strip() for l in open(sys.argv[i + 1]) if l.strip()]
for pair in pairs:
    o, _, nw = pair.partition("=")
    assert o in old and nw in new and nw not in old, "no such pair of kernels: " + pair
    old[nw] = old.pop(o)
    print(f"compared as one kernel: {o}  ->  {nw}")
common = sorted(set(old) & set(new))
differ = [k for k in common if old[k] != new[k]]
for title, names in (("removed", sorted(set(old) - set(new))), ("added", sorted(set(new) - set(old))), ("DIFFER", differ)):
    print(f"{title}: {len(names)}")
    for k in names:
        print("   ", k, f"({len(old[k])} -> {len(new[k])} instructions)" if title == "DIFFER" else "")
        if title == "DIFFER" and "--opcodes" in sys.argv:
            ho, hn = opcodes(old[k]), opcodes(new[k])
            print("        " + ("; ".join(f"{op} {ho[op]} -> {hn[op]}" for op in sorted(set(ho) | set(hn)) if ho[op] != hn[op]) or "(every opcode count unchanged: order or registers only)"))
print(f"identical: {len(common) - len(differ)} of {len(common)} common kernels, {sum(len(old[k]) for k in common)} instructions;"
      f" library size {os.path.getsize(sys.argv[1])} -> {os.path.getsize(sys.argv[2])} bytes")
sys.exit(1 if differ else 0)
