"""Structure of the headline step kernel's code in a built libmwstep.so.  CPU only.

    python scripts/step_kernel_isa.py [path/to/libmwstep.so]

The headline kernel is the closed-loop CartPole step of bench.py:
vecenv_step_kernel<N=2, KIND=0, DUAL=false, CONS=true, ROLLOUT=false,
BAKED=cartpole, RAND=false> (64-thread workgroups where the workgroup size is
a template argument; the single-substep instantiation where the library has
one: bench.py runs one substep per step).  The script pulls the gfx950 code objects out of the
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
  path_instructions         helper-wave kernels: per role ("wave0", "helper") the
                            instructions issued and branches taken along the
                            common path, entry -> s_endpgm (wave 0: a lane
                            inside W, no limit row, no lane done); see _walk

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
HEADLINE = re.compile(r"^_ZN2mw3dev18vecenv_step_kernelILi2ELi0ELb0ELb1ELb0ELi[1-9]\d*ELb0E(Li64E(Lb[01]E(Lb1E)?)?)?EEv\w*$")
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


class PathError(Exception):
    """The walk met code that the branch rules of _walk do not describe."""


def _target(body, addr, at, k):
    imm = int(body[k][1].split()[-1], 0) & 0xFFFF
    return at[addr[k] + 4 + 4 * (imm - 0x10000 if imm & 0x8000 else imm)]


def _walk(body, addr, at, role):
    """Instructions issued and branches taken along the common path of one
    role of a helper-wave kernel, entry -> s_endpgm.  role "wave0": the
    physics wave with a lane inside W, no limit row active and no lane done;
    "helper": the wave that draws the reset state.  The branch decisions:

      * a uniform branch (scc / vcc) from which only one side leads to the
        role's work (wave 0: a global store; helper: an LDS write) goes there;
      * any other uniform branch falls through: the code it could skip depends
        on an argument and runs (substeps >= 1, reward shaping on) -- unless
        falling through repeats an instruction of the path, the second trip
        of a loop, which runs once: then it is taken;
      * s_cbranch_execz is taken: the lanes it guards are those with a limit
        row, done lanes or lanes whose episode changed, and there are none --
        except behind the `w < W` test, recognised as the only signed integer
        vector compare (v_cmp_gt_i32): those lanes exist, it falls through;
      * s_cbranch_execnz (a lane loop's back edge) falls through.

    The result is checked against what the path must contain (the barrier;
    wave 0: stores and no LDS read; helper: an LDS write and no store)."""
    ops = [op for op, _ in body]
    work = "global_store" if role == "wave0" else "ds_write"

    def reaches_work(k0):
        seen, todo = set(), [k0]
        while todo:
            k = todo.pop()
            if k in seen or k >= len(body):
                continue
            seen.add(k)
            if ops[k].startswith(work):
                return True
            if ops[k] == "s_endpgm":
                continue
            if ops[k] == "s_branch":
                todo.append(_target(body, addr, at, k))
                continue
            if ops[k].startswith("s_cbranch"):
                todo.append(_target(body, addr, at, k))
            todo.append(k + 1)
        return False

    def mask_writer(path, mask):
        for k in reversed(path):
            if body[k][1].split(",")[0].strip() == mask and not ops[k].startswith("s_cbranch"):
                return ops[k]
        return ""

    path, on_path, taken, k = [], set(), 0, 0
    while True:
        if k >= len(body) or len(path) > 4 * len(body):
            raise PathError(f"{role}: the walk left the kernel or does not end")
        path.append(k)
        on_path.add(k)
        op = ops[k]
        if op == "s_endpgm":
            break
        if op == "s_branch":
            k, taken = _target(body, addr, at, k), taken + 1
            continue
        if not op.startswith("s_cbranch"):
            k += 1
            continue
        tgt = _target(body, addr, at, k)
        if op in ("s_cbranch_execz", "s_cbranch_execnz"):
            take = False
            if op == "s_cbranch_execz":
                # the instruction that set exec: s_and_saveexec_b64 d, m / s_and_b64 exec, exec, m
                setter = next((j for j in reversed(path[:-1]) if ops[j].startswith("s_and_saveexec") or
                               (ops[j] == "s_and_b64" and body[j][1].startswith("exec, exec,"))), None)
                if setter is None:
                    raise PathError(f"{role}: no exec mask in front of {op}")
                mask = body[setter][1].split(",")[-1].strip()
                take = not mask_writer(path[:path.index(setter)], mask).startswith("v_cmp_gt_i32")
        else:
            sides = [reaches_work(tgt), reaches_work(k + 1)]
            if sides[0] != sides[1]:
                take = sides[0]
            else:
                take = (k + 1) in on_path
        if take:
            k, taken = tgt, taken + 1
        else:
            k += 1
    pops = [ops[j] for j in path]
    ok = "s_barrier" in pops
    if role == "wave0":
        ok = ok and any(p.startswith("global_store") for p in pops) and not any(p.startswith("ds_read") for p in pops)
    else:
        ok = ok and any(p.startswith("ds_write") for p in pops) and not any(p.startswith("global_store") for p in pops)
    if not ok:
        raise PathError(f"{role}: the walked path is not the role's common path")
    return {"instructions": len(path), "taken_branches": taken,
            "stores": sum(p.startswith("global_store") for p in pops)}


def path_instructions(lib_path, pattern=HEADLINE):
    """{"wave0": {...}, "helper": {...}} of the kernel that `pattern` selects:
    see _walk.  None without the LLVM tools; {} if there is no such kernel."""
    res = analyse(lib_path, pattern)
    return res["path_instructions"] if res else res


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
    try:
        paths = {role: _walk(body, addr, at, role) for role in ("wave0", "helper")} if lds_bytes else None
    except PathError as e:
        paths = {"error": str(e)}
    return {
        "path_instructions": paths,
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
