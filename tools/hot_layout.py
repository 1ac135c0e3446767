"""Code layout of the ray loops in the built device code object (CPU only).

Where the run kernel's loops lie: for a named kernel, its size, every loop
that holds cell-cache refills (the groups of global_load_lds instructions of
CachedStaticBG's refill), each loop's span -- the innermost backward branch
that encloses the refills, from its target to the branch -- the offsets of
the refills and the number of instructions inside the span.  The ray loop is
the loop with six 24-load refills (one per RK stage); the other loops are the
latency mode's (quad_run: the launch's heavy rays, and the drain-time
hand-off).

A common path that lies contiguously and is smaller than the instruction
cache cannot collide with itself at any placement of the code object; a loop
whose span is inflated by the bodies of rarely taken branches can (DESIGN.md
section 9, "Code layout").  tests/test_hot_layout_host.py gates the span.

The tool reads branch targets and the positions of the refills from
llvm-objdump's disassembly, and nothing else.

  python tools/hot_layout.py [--lib librwrt.so | --compile [--defs "-DX=1"]] [--kernel static|guarded|...]
                             [--json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rossby-wave-ray-tracing_amd")
CSRC = os.path.join(PKG, "csrc")
LLVM = os.environ.get("RWRT_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNELS = {
    "static": "_ZN4rwrt15rk45_run_kernelINS_8StaticBGELb0ELb1EEEvNS_7RunArgsIT_EE",
    "guarded": "_ZN4rwrt15rk45_run_kernelINS_8StaticBGELb0ELb0EEEvNS_7RunArgsIT_EE",
    "back_static": "_ZN4rwrt20rk45_run_back_kernelILb1EEEvNS_7RunArgsINS_8StaticBGEEE",
    "back_guarded": "_ZN4rwrt20rk45_run_back_kernelILb0EEEvNS_7RunArgsINS_8StaticBGEEE",
    "stack": "_ZN4rwrt15rk45_run_kernelINS_7StackBGELb0ELb0EEEvNS_7RunArgsIT_EE",
}
GATED = ("static", "guarded")
# The gate (tests/test_hot_layout_host.py): the ray loop's span.  The common
# path is ~40 KB (tools/hot_count.py: ~6 100 instructions of ~6.5 B), the six
# refills are inline; 48 KiB leaves room below a 64 KB instruction cache that
# two CUs running the same loop share.
SPAN_LIMIT = 48 * 1024
REFILL_LOADS = 24    # global_load_lds per refill of the ray loop (6 chunks x 4 rows)
REFILL_GAP = 1024    # two loads further apart than this belong to different refills


def tools_present():
    return all(os.path.exists(os.path.join(LLVM, t)) for t in
               ("clang-offload-bundler", "llvm-objdump", "llvm-objcopy"))


def _run(*cmd):
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


def code_objects(path, tmp):
    """The gfx950 code objects of a shared library or host object file (one per translation unit)."""
    head = open(path, "rb").read(len(MAGIC))
    if head[:4] == b"\x7fELF" and head[18:20] == b"\xe0\x00":   # (EM_AMDGPU: a code object itself)
        return [path]
    if head == MAGIC:   # (hipcc --cuda-device-only -c: the bundle itself)
        data = open(path, "rb").read()
    else:
        fat = os.path.join(tmp, "fatbin")
        _run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path)
        data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = []
    for i, s in enumerate(starts):
        piece = os.path.join(tmp, f"bundle{i}")
        with open(piece, "wb") as f:
            f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = os.path.join(tmp, f"co{i}")
        _run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + piece,
             "--targets=" + TARGET, "--output=" + co)
        out.append(co)
    return out


def compile_code_object(defs, tmp):
    """A fresh device-only compile of rwrt.hip with the Makefile's flags."""
    co = os.path.join(tmp, "rwrt.co")
    _run("/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
         "-fno-fast-math", "-fPIC", "-Wall", "-fconstexpr-steps=20000000", "-I" + os.path.join(ROOT, "include"),
         "--cuda-device-only", "-c", *defs, "-o", co, os.path.join(CSRC, "rwrt.hip"))
    return code_objects(co, tmp)


_FUNC = re.compile(r"^([0-9a-f]+) <([^>]+)>:")
_INSN = re.compile(r"^\s+(\S+)\s.*//\s*([0-9A-Fa-f]+):")
_INSN0 = re.compile(r"^\s+(\S+)\s*//\s*([0-9A-Fa-f]+):")
_TARGET = re.compile(r"<([^>+]+)\+0x([0-9a-f]+)>\s*$")


def disassemble(co, name):
    """[(offset, mnemonic, branch target offset or None)] of one kernel, or None if the
    code object has no such kernel."""
    p = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn",
                        "--disassemble-symbols=" + name, co], check=True, capture_output=True, text=True)
    base, insns = None, []
    for line in p.stdout.split("\n"):
        m = _FUNC.match(line)
        if m:
            if m.group(2) == name:
                base = int(m.group(1), 16)
            elif base is not None:
                break
            continue
        if base is None:
            continue
        m = _INSN.match(line) or _INSN0.match(line)
        if not m:
            continue
        op, off = m.group(1), int(m.group(2), 16) - base
        tgt = None
        if op.startswith(("s_cbranch", "s_branch")):
            t = _TARGET.search(line)
            if t and t.group(1) == name:
                tgt = int(t.group(2), 16)
            elif line.rstrip().endswith("<" + name + ">"):
                tgt = 0
        insns.append((off, op, tgt))
    return (base, insns) if base is not None and insns else None


def layout(base, insns):
    size = insns[-1][0] + 4   # (to the last instruction; the padding behind s_endpgm is not code)
    offs = [o for o, _, _ in insns]
    loads = [o for o, op, _ in insns if op.startswith("global_load_lds")]
    groups = []   # refills: [first offset, last offset, loads]
    for o in loads:
        if groups and o - groups[-1][1] <= REFILL_GAP:
            groups[-1][1] = o
            groups[-1][2] += 1
        else:
            groups.append([o, o, 1])
    # a loop evaluates the RHS six times (the RK stages), each with its refill: six
    # consecutive refills of one size are one loop's, and the loop is the innermost
    # backward branch that encloses all six (the bodies laid out behind a loop branch
    # back into it: those edges are wider than the loop's own)
    back = [(o, t) for o, _, t in insns if t is not None and t <= o]
    res = []
    for i in range(0, len(groups) - 5, 6):
        gs = groups[i:i + 6]
        if len({g[2] for g in gs}) != 1:
            raise SystemExit(f"refills {[g[2] for g in groups]}: not runs of six of one size")
        enclosing = [(o + 4 - t, t, o) for o, t in back if t <= gs[0][0] and gs[-1][1] <= o]
        if not enclosing:
            continue
        _, t, o = min(enclosing)
        res.append({"start": t, "end": o, "span": o + 4 - t, "instructions": sum(1 for x in offs if t <= x <= o),
                    "refills": [g[0] for g in gs], "refill_last": [g[1] for g in gs],
                    "refill_loads": [g[2] for g in gs]})
    ray = [l for l in res if l["refill_loads"][0] == REFILL_LOADS]
    return {"address": base, "size": size, "instructions": len(insns),
            "ray_loop": ray[0] if len(ray) == 1 else None,
            "quad_loops": [l for l in res if l["refill_loads"][0] != REFILL_LOADS]}


def layouts(path=None, kernels=GATED, defs=None):
    """The layouts of kernels of the built library (path), or of a fresh compile (path None)."""
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        cos = code_objects(path, tmp) if path else compile_code_object(defs or [], tmp)
        for kernel in kernels:
            name = KERNELS.get(kernel, kernel)
            for co in cos:
                d = disassemble(co, name)
                if d:
                    r = layout(*d)
                    r["kernel"] = kernel
                    res.append(r)
                    break
            else:
                raise SystemExit(f"no kernel {name} in {path or 'the compile'}")
    return res


def show(r):
    kb = lambda b: f"{b / 1024:.1f}"
    print(f"kernel {r['kernel']}: at 0x{r['address']:x}, {r['size']} bytes, {r['instructions']} instructions")

    def loop(tag, l):
        print(f"  {tag}: +0x{l['start']:x} .. +0x{l['end']:x}  span {l['span']} B ({kb(l['span'])} KB), "
              f"{l['instructions']} instructions")
        print("    refills (KB from the kernel's start; loads): " +
              "  ".join(f"{kb(o)} ({n})" for o, n in zip(l["refills"], l["refill_loads"])))
        print("    refills from the loop's start (KB): " + " ".join(kb(o - l["start"]) for o in l["refills"]))
    if r["ray_loop"]:
        loop("ray loop", r["ray_loop"])
    else:
        print("  ray loop: not found (no loop with six 24-load refills)")
    for i, l in enumerate(r["quad_loops"]):
        loop(f"quad loop {i}", l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(PKG, "librwrt.so"))
    ap.add_argument("--compile", action="store_true", help="compile rwrt.hip afresh (device only)")
    ap.add_argument("--defs", default="")
    ap.add_argument("--kernel", action="append", help="a name of KERNELS or a mangled symbol (default: static, guarded)")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not tools_present():
        sys.exit("clang-offload-bundler / llvm-objdump / llvm-objcopy not found under " + LLVM)
    for r in layouts(None if args.compile else args.lib, args.kernel or GATED, args.defs.split()):
        if args.json:
            print(json.dumps(r))
        else:
            show(r)


if __name__ == "__main__":
    main()
