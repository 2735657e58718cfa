#!/usr/bin/env python3
"""tools/shipped_isa.py [REGEX] -- what is INSIDE a built libwhvi_hip.so: per kernel, the register / scratch / LDS figures
of the gfx950 code objects' metadata, and (for kernels whose demangled name matches REGEX) the disassembly with the issue
pattern of its 16-byte stores.  Needs no GPU and no recompilation: it reads the shipped binary (llvm-objdump --offloading,
llvm-readelf --notes, llvm-objdump -d).  tests/test_build.py uses it to pin the occupancy budgets and the store issue forms
the streaming kernels were tuned for (9 % of the headline rate hangs on how 16 stores are issued).

    python tools/shipped_isa.py 'fwht_rows_kernel<float, 12, 16, 0, false, true, 256, 1, false>'
    python tools/shipped_isa.py --lib whvi_amd/_exp/libwhvi_hip_x.so 'wbar_fwd_kernel<float, 11'
    python tools/shipped_isa.py --against ../parent/whvi_amd/libwhvi_hip.so     # did a source change move any shipped code?

--against OTHER_LIB compares the library with another build of it, kernel by kernel: the kernels only one of them has, those
whose metadata differs, those whose instruction text differs and the code objects whose .rodata (the kernel descriptors)
differs; the exit status is non-zero if there is any.  It compares text and metadata, not bytes: two builds of the same
sources differ in bytes."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
DEFAULT_LIB = os.path.join(ROOT, "whvi_amd", "libwhvi_hip.so")


class ShippedLibrary:
    """Kernels of one built library.  ``kernels``: demangled name -> dict(mangled, vgprs, agprs, sgprs, scratch, lds, code_object)."""

    def __init__(self, lib=DEFAULT_LIB):
        self.tmp = tempfile.mkdtemp(prefix="whvi_isa_")
        copy = os.path.join(self.tmp, "lib.so")
        shutil.copy(lib, copy)                      # the extractor writes its bundles next to the file it reads
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", copy], check=True, capture_output=True, cwd=self.tmp)
        self.kernels = {}
        mangled_of = {}
        for name in sorted(os.listdir(self.tmp)):
            if "gfx950" not in name:
                continue
            path = os.path.join(self.tmp, name)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], check=True, capture_output=True, text=True).stdout
            # one YAML block per kernel under amdhsa.kernels: take the scalar fields we need from each "- .args:" item
            for block in re.split(r"\n  - \.", notes):
                m = re.search(r"\.name:\s+(\S+)", block)
                v = re.search(r"\.vgpr_count:\s+(\d+)", block)
                if not m or not v:
                    continue
                field = lambda key, d=0: int((re.search(r"\.%s:\s+(\d+)" % key, block) or [None, d])[1])   # noqa: E731
                mangled_of[m.group(1)] = dict(mangled=m.group(1), vgprs=int(v.group(1)), agprs=field("agpr_count"),
                                              sgprs=field("sgpr_count"), scratch=field("private_segment_fixed_size"),
                                              lds=field("group_segment_fixed_size"), code_object=path)
        names = list(mangled_of)
        pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        for mangled, p in zip(names, pretty):
            p = re.sub(r"\(.*$", "", p.strip())     # "void whvi::k<...>(args)" -> "whvi::k<...>"
            p = re.sub(r"^void ", "", p)
            self.kernels[p] = mangled_of[mangled]

    def close(self):
        shutil.rmtree(self.tmp, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def find(self, name):
        """The kernel whose demangled name is exactly ``name`` (KeyError with near misses otherwise)."""
        if name in self.kernels:
            return self.kernels[name]
        family = name.split("<")[0]
        near = [k for k in self.kernels if k.startswith(family + "<")][:8]
        raise KeyError(f"{name} is not in the shipped library; same family: {near}")

    def ops(self, name):
        """[(mnemonic, operand text)] of the kernel's instructions, in program order."""
        k = self.find(name)
        out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", f"--disassemble-symbols={k['mangled']}",
                              k["code_object"]], check=True, capture_output=True, text=True).stdout
        ops = []
        for line in out.splitlines():
            m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*(//.*)?$", line)
            if m and not line.strip().startswith(("//", ";")):
                ops.append((m.group(1), m.group(2)))
        return ops


def store_runs(ops, mnemonic):
    """Lengths of the maximal runs of consecutive ``mnemonic`` instructions (16-byte stores issued back to back)."""
    runs, cur = [], 0
    for op, _ in ops:
        if op == mnemonic:
            cur += 1
        else:
            if cur:
                runs.append(cur)
            cur = 0
    if cur:
        runs.append(cur)
    return runs


_INSN = re.compile(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//\s*([0-9A-F]+):")
_SYMBOL = re.compile(r"^[0-9a-f]+ <(\S+)>:")
_WIDE_STORE = re.compile(r"(global|flat|scratch|buffer)_store_(dwordx3|dwordx4|b96|b128)$")


def _vgprs(operand):
    m = re.fullmatch(r"v(\d+)", operand) or re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    if not m:
        return set()
    return set(range(int(m.group(1)), int(m.group(m.lastindex)) + 1))


def store_data_hazards(code_object, wait_states=2):
    """Stores of more than 64 bits whose data VGPRs a VALU instruction overwrites fewer than ``wait_states`` wait states later
    (every instruction is one, ``s_nop N`` is N + 1; branches are followed).  The hardware may then store the NEW value: gfx950
    needs two wait states there.  hipcc pads the stores it emits; an inline-asm store has to carry its own ``s_nop``.
    Returns [(mangled kernel, store, the VALU instruction, wait states between them)]."""
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", code_object], check=True, capture_output=True,
                          text=True).stdout
    ins, index, symbol = [], {}, None
    for line in text.splitlines():
        s = _SYMBOL.match(line)
        if s:
            symbol = s.group(1)
            continue
        m = _INSN.match(line)
        if m:
            index[int(m.group(3), 16)] = len(ins)
            ins.append((m.group(1), m.group(2), int(m.group(3), 16), symbol))
    found = []
    for i, (op, args, _, symbol) in enumerate(ins):
        if not _WIDE_STORE.match(op):
            continue
        operands = [t.strip() for t in re.split(r",\s*(?![^\[]*\])", args)]
        data = _vgprs(operands[0] if op.startswith("buffer_") else operands[1])
        todo, seen = [(i + 1, 0)], set()
        while todo:
            j, waited = todo.pop()
            if j >= len(ins) or waited >= wait_states or (j, waited) in seen:
                continue
            seen.add((j, waited))
            nop, nargs, addr, _ = ins[j]
            if nop.startswith("v_") and _vgprs(nargs.split(",")[0].strip()) & data:
                found.append((symbol, f"{op} {args}", f"{nop} {nargs}", waited))
                continue
            if nop == "s_endpgm":
                continue
            step = int(nargs) + 1 if nop == "s_nop" else 1
            if nop == "s_branch" or nop.startswith("s_cbranch"):
                imm = int(nargs.split()[0])
                target = addr + 4 + 4 * (imm - 65536 if imm >= 32768 else imm)
                if target in index:
                    todo.append((index[target], waited + step))
                if nop == "s_branch":
                    continue
            todo.append((j + 1, waited + step))
    return found


def compare(lib, other):
    """Differences between two built libraries as dict(kernels, only_in_one, metadata, instructions, rodata): the number of
    kernels both have, and the names (demangled; rodata: one kernel of the code object) of what differs."""
    fields = ("vgprs", "agprs", "sgprs", "scratch", "lds")

    def contents(shipped):
        name_of = {k["mangled"]: name for name, k in shipped.kernels.items()}
        text, rodata = {}, {}
        for obj in sorted({k["code_object"] for k in shipped.kernels.values()}):
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", obj], check=True, capture_output=True,
                                 text=True).stdout
            symbol = None
            for line in dis.splitlines():
                s = _SYMBOL.match(line)
                m = None if s else re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*(//.*)?$", line)
                if s:
                    symbol = name_of.get(s.group(1))
                    text.setdefault(symbol, [])
                elif m and symbol is not None:
                    text[symbol].append((m.group(1), m.group(2)))
            first = min(n for n, k in shipped.kernels.items() if k["code_object"] == obj)
            rodata[first] = subprocess.run([f"{LLVM}/llvm-objdump", "-s", "-j", ".rodata", obj], check=True, capture_output=True,
                                           text=True).stdout.split("Contents of section", 1)[-1]
        return text, rodata

    with ShippedLibrary(lib) as a, ShippedLibrary(other) as b:
        (text_a, ro_a), (text_b, ro_b) = contents(a), contents(b)
        both = sorted(set(a.kernels) & set(b.kernels))
        return dict(kernels=len(both), only_in_one=sorted(set(a.kernels) ^ set(b.kernels)),
                    metadata=[n for n in both if any(a.kernels[n][f] != b.kernels[n][f] for f in fields)],
                    instructions=[n for n in both if text_a.get(n) != text_b.get(n) or not text_a.get(n)],
                    rodata=sorted(n for n in set(ro_a) | set(ro_b) if ro_a.get(n) != ro_b.get(n)))


def main():
    args = [a for a in sys.argv[1:]]
    lib = DEFAULT_LIB
    if "--lib" in args:
        i = args.index("--lib")
        lib = args[i + 1]
        del args[i:i + 2]
    if "--against" in args:
        diff = compare(lib, args[args.index("--against") + 1])
        print(f"{diff['kernels']} kernels in both {lib} and {args[args.index('--against') + 1]}")
        for what in ("only_in_one", "metadata", "instructions", "rodata"):
            print(f"{what}: {len(diff[what])} differ" + "".join(f"\n    {n}" for n in diff[what]))
        sys.exit(1 if any(diff[w] for w in ("only_in_one", "metadata", "instructions", "rodata")) else 0)
    pattern = re.compile(args[0]) if args else None
    with ShippedLibrary(lib) as shipped:
        print(f"{len(shipped.kernels)} kernels in {lib}; with scratch: {sum(1 for k in shipped.kernels.values() if k['scratch'])}")
        for name, k in sorted(shipped.kernels.items()):
            if pattern is None or not pattern.search(name):
                continue
            ops = shipped.ops(name)
            print(name)
            print("   ", {f: k[f] for f in ("vgprs", "agprs", "sgprs", "scratch", "lds")}, f"{len(ops)} instructions")
            for mnemonic in ("buffer_store_dwordx4", "global_store_dwordx4"):
                runs = store_runs(ops, mnemonic)
                if runs:
                    print(f"    {mnemonic}: {sum(runs)} stores in runs of {runs}")


if __name__ == "__main__":
    main()
