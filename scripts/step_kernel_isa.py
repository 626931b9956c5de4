"""Structure of the headline step kernel's code in a built libmwstep.so.  CPU only.

    python scripts/step_kernel_isa.py [path/to/libmwstep.so]

The headline kernel is the closed-loop CartPole step of bench.py:
vecenv_step_kernel<N=2, KIND=0, DUAL=false, CONS=true, ROLLOUT=false,
BAKED=cartpole, RAND=false> (64-thread workgroups where the workgroup size is
a template argument).  The script pulls the gfx950 code objects out of the
library, disassembles that kernel with the ROCm LLVM tools and prints, as JSON:

  kernarg_size              bytes, from the kernel descriptor
  kernarg_preload_dwords    user SGPRs preloaded from the kernarg segment
  s_load                    scalar loads in the kernel body
  lgkm_waits_before_first_global_load
  s_load_after_first_vmcnt_wait
  global_loads, global_loads_before_first_vmcnt_wait
  vmcnt_waits_after_first_store   s_waitcnt vmcnt(..) that can execute after a
                            global store (branch targets followed): a store
                            waiting for the acknowledgement of earlier ones
  lds_bytes                 group_segment_fixed_size of the kernel descriptor
                            (> 0: the workgroup has a helper wave)

With preloading, the compiler puts a 256-byte compatibility prologue in front
of the body (it loads the preloaded arguments by hand, for firmware that does
not preload; firmware that does enters 256 bytes later).  The counts are of
the body; the prologue's own loads are reported as prologue_s_load.

It reports structure only, no timing.  Exit status 2: the LLVM tools (or the
kernel) were not found."""

import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "gym-ignition_amd", "libmwstep.so")
HEADLINE = re.compile(r"^_ZN2mw3dev18vecenv_step_kernelILi2ELi0ELb0ELb1ELb0ELi[1-9]\d*ELb0E(Li64E(Lb[01]E)?)?EEv\w*$")
# every closed-loop (ROLLOUT == false) instantiation
CLOSED_LOOP = re.compile(r"^_ZN2mw3dev18vecenv_step_kernelILi\d+ELi\d+ELb[01]ELb[01]ELb0E\w*$")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def llvm_tools():
    """(llvm-readelf, llvm-objdump) of the ROCm install, or None."""
    for base in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if not base:
            continue
        d = os.path.join(base, "llvm", "bin")
        pair = (os.path.join(d, "llvm-readelf"), os.path.join(d, "llvm-objdump"))
        if all(os.access(p, os.X_OK) for p in pair):
            return pair
    return None


def code_objects(lib_bytes, arch="gfx950"):
    """The device ELF images of every offload bundle in the library."""
    out, i = [], lib_bytes.find(BUNDLE_MAGIC)
    while i >= 0:
        (n,) = struct.unpack_from("<Q", lib_bytes, i + len(BUNDLE_MAGIC))
        p = i + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", lib_bytes, p)
            triple = lib_bytes[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if arch in triple and size:
                out.append(lib_bytes[i + off:i + off + size])
        i = lib_bytes.find(BUNDLE_MAGIC, i + len(BUNDLE_MAGIC))
    return out


def elf_bytes_at(elf, addr, n):
    """n bytes at virtual address addr of a little-endian ELF64 image."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    for k in range(shnum):
        sh = shoff + k * shentsize
        sh_type, = struct.unpack_from("<I", elf, sh + 4)
        sh_addr, sh_offset, sh_size = struct.unpack_from("<QQQ", elf, sh + 0x10)
        if sh_type != 8 and sh_addr <= addr and addr + n <= sh_addr + sh_size:  # 8: SHT_NOBITS
            return elf[sh_offset + addr - sh_addr:sh_offset + addr - sh_addr + n]
    raise ValueError(f"address {addr:#x} is in no section")


def analyse(lib_path, pattern=HEADLINE, every=False):
    """The counts of the first kernel (sorted by name) whose symbol matches
    `pattern`; with every=True a list, one entry per matching kernel."""
    tools = llvm_tools()
    if tools is None:
        return None
    found = []
    readelf, objdump = tools
    with open(lib_path, "rb") as f:
        lib_bytes = f.read()
    with tempfile.TemporaryDirectory() as tmp:
        for k, elf in enumerate(code_objects(lib_bytes)):
            path = os.path.join(tmp, f"co{k}.elf")
            with open(path, "wb") as f:
                f.write(elf)
            syms = subprocess.run([readelf, "-s", "--wide", path], capture_output=True, text=True, check=True).stdout
            funcs, kds = {}, {}
            for line in syms.splitlines():
                c = line.split()
                if len(c) == 8 and c[3] == "FUNC" and pattern.match(c[7]):
                    funcs[c[7]] = int(c[1], 16)
                elif len(c) == 8 and c[3] == "OBJECT" and c[7].endswith(".kd"):
                    kds[c[7][:-3]] = int(c[1], 16)
            if not funcs:
                continue
            for name in sorted(funcs):
                found.append(_counts(lib_path, elf, path, objdump, name, funcs[name], kds[name]))
                if not every:
                    return found[0]
    return found if every else {}


def _counts(lib_path, elf, path, objdump, name, func_at, kd_at):
    kd = elf_bytes_at(elf, kd_at, 64)   # amd_kernel_code descriptor, 64 bytes
    lds_bytes, = struct.unpack_from("<I", kd, 0)   # group_segment_fixed_size
    kernarg_size, = struct.unpack_from("<I", kd, 8)
    preload, = struct.unpack_from("<H", kd, 58)
    preload &= 0x7F
    dis = subprocess.run([objdump, "-d", f"--disassemble-symbols={name}", path], capture_output=True,
                         text=True, check=True).stdout
    insts = []
    for line in dis.splitlines():
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*// ([0-9A-Fa-f]+):", line)
        if m:
            insts.append((int(m.group(3), 16), m.group(1), m.group(2)))
    body_at = func_at + (256 if preload else 0)
    body = [(op, args) for a, op, args in insts if a >= body_at]
    prologue = [(op, args) for a, op, args in insts if a < body_at]
    ops = [op for op, _ in body]
    vm_wait = [op == "s_waitcnt" and "vmcnt" in args for op, args in body]
    first_gl = next((k for k, op in enumerate(ops) if op.startswith("global_load")), len(ops))
    first_vm = next((k for k, v in enumerate(vm_wait) if v), len(ops))
    # vector-memory waits that can EXECUTE after a global store: reachability
    # over the branch targets, not position in the listing (the helper wave's
    # code lies behind wave 0's stores in the file and never runs after them)
    addr = [a for a, _, _ in insts if a >= body_at]
    at = {a: k for k, a in enumerate(addr)}
    succ = []
    for k, (op, args) in enumerate(body):
        nxt = [] if op in ("s_endpgm", "s_branch") or k + 1 == len(body) else [k + 1]
        if op == "s_branch" or op.startswith("s_cbranch"):
            imm = int(args.split()[-1], 0) & 0xFFFF
            nxt.append(at[addr[k] + 4 + 4 * (imm - 0x10000 if imm & 0x8000 else imm)])
        succ.append(nxt)
    todo = [n for k, op in enumerate(ops) if op.startswith("global_store") for n in succ[k]]
    after_store = set()
    while todo:
        k = todo.pop()
        if k not in after_store:
            after_store.add(k)
            todo.extend(succ[k])
    return {
        "library": os.path.basename(lib_path),
        "kernel": name,
        "kernarg_size": kernarg_size,
        "kernarg_preload_dwords": preload,
        "lds_bytes": lds_bytes,
        "instructions": len(body),
        "s_load": sum(op.startswith("s_load") for op in ops),
        "prologue_s_load": sum(op.startswith("s_load") for op, _ in prologue),
        "lgkm_waits_before_first_global_load": sum(
            op == "s_waitcnt" and "lgkmcnt" in args for op, args in body[:first_gl]),
        "s_load_after_first_vmcnt_wait": sum(op.startswith("s_load") for op in ops[first_vm:]),
        "global_loads_before_first_vmcnt_wait": sum(op.startswith("global_load") for op in ops[:first_vm]),
        "global_loads": sum(op.startswith("global_load") for op in ops),
        "vmcnt_waits_after_first_store": sum(vm_wait[k] for k in after_store),
    }


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_LIB
    res = analyse(lib)
    if res is None:
        print("llvm-readelf / llvm-objdump not found under $ROCM_PATH or /opt/rocm", file=sys.stderr)
        return 2
    if not res:
        print(f"no headline step kernel in {lib}", file=sys.stderr)
        return 2
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
