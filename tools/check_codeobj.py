"""Resource and call report of the gfx950 kernels inside a hipcc-built shared
library or object (test infrastructure: tests/test_codeobj.py).

The fused append + stream kernel (k_inc_stream) relies on producers and cell
workgroups being resident together and on code with no out-of-line calls: an
outlined producer once stalled the hand-off for seconds.
This module extracts the code object (.hip_fatbin -> clang-offload-bundler),
reads the AMDGPU metadata note (VGPRs, spills, LDS) and counts call
instructions (s_swappc_b64) in each kernel's disassembly.

usage: python tools/check_codeobj.py mfgp_coverage_amd/libmfgp_hip.so
       python tools/check_codeobj.py compare OLD.so NEW.so   (two builds, kernel by kernel: a
       refactor of the kernel sources is checked by the compiler emitting the same code)
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

import yaml

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(path, workdir):
    fat = os.path.join(workdir, "fatbin.bin")
    co = os.path.join(workdir, "gfx950.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", path, os.path.join(workdir, "x")],
                   check=True, capture_output=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}",
                    f"--input={fat}", f"--output={co}"], check=True, capture_output=True)
    return co


def metadata(co):
    out = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    y = out[out.index("---"):]
    y = y[: y.index("\n...")] if "\n..." in y else y
    return yaml.safe_load(y)["amdhsa.kernels"]


def calls(co):
    """{kernel symbol: number of s_swappc_b64 in its body}."""
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = 0
        elif cur and "s_swappc_b64" in line:
            out[cur] += 1
    return out


def disassembly(co):
    """{kernel symbol: [(address, mnemonic, operands, branch target address or None)]}."""
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                         text=True).stdout
    out, cur, base = {}, None, 0
    for line in dis.splitlines():
        m = re.match(r"^([0-9a-f]+) <([^>]+)>:", line)
        if m:
            cur, base = out.setdefault(m.group(2), []), int(m.group(1), 16)
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if cur is not None and m:
            t = re.search(r"<[^+>]+\+0x([0-9a-f]+)>", line)
            cur.append((int(m.group(3), 16), m.group(1), m.group(2), base + int(t.group(1), 16) if t else None))
    return out


VMEM_LOAD = ("global_load", "buffer_load", "flat_load")


def poll_iterations(ins):
    """The hand-off waits' poll iterations of one kernel. Every bounded spin sleeps
    (s_sleep) between polls, so each s_sleep marks one spin loop: the instructions
    from the target of the first branch after the s_sleep that jumps back to it or
    above (the loop's back edge; the compiler may put the bound's test on it) up to
    that branch. Returns one record per s_sleep: the loop's vector loads (its polls
    of the hand-off words); whether all carry sc1 (device scope, L2-coherent across
    the XCDs: a flag is never served from a stale line); and whether every one of
    them is followed by an s_waitcnt vmcnt(0) before the next conditional branch
    (the branch reads the flag's value, so nothing after the exit is issued before
    the flag was seen)."""
    at = {a: i for i, (a, _, _, _) in enumerate(ins)}
    out = []
    for i, (addr, op, _, _) in enumerate(ins):
        if op != "s_sleep":
            continue
        head = br = None
        for j in range(i + 1, min(len(ins), i + 400)):
            _, op2, _, tgt = ins[j]
            if op2.startswith(("s_branch", "s_cbranch")) and tgt is not None and tgt <= addr and tgt in at:
                head, br = at[tgt], j
                break
        body = ins[head:br + 1] if head is not None else []
        loads, waited, pending = [], True, False
        for _, op2, args, _ in body:
            if op2.startswith(VMEM_LOAD):
                loads.append((op2, args))
                pending = True
            elif op2 == "s_waitcnt" and "vmcnt(0)" in args:
                pending = False
            elif op2.startswith("s_cbranch") and pending:
                waited = False
        out.append({"loads": loads, "sc1": bool(loads) and all(re.search(r"\bsc1\b", a) for _, a in loads),
                    "waited": waited and bool(loads)})
    return out


def hand_off_report(path, names):
    """{kernel: poll iterations} for the kernels whose symbol contains one of `names`."""
    with tempfile.TemporaryDirectory() as td:
        dis = disassembly(code_object(path, td))
    return {k: poll_iterations(v) for k, v in dis.items() if any(n in k for n in names)}


BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path, workdir):
    """The gfx950 code object of every translation unit: the library is linked without
    -fgpu-rdc, so its .hip_fatbin section holds one offload bundle per unit, one after
    the other (code_object above unbundles the first: mfgp_kernels.hip's)."""
    fat = os.path.join(workdir, "fatbin_all.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", path, os.path.join(workdir, "y")],
                   check=True, capture_output=True)
    with open(fat, "rb") as fh:
        blob = fh.read()
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), blob)]
    cos = []
    for i, st in enumerate(starts):
        part = os.path.join(workdir, f"bundle{i}.bin")
        co = os.path.join(workdir, f"gfx950_{i}.co")
        with open(part, "wb") as fh:
            fh.write(blob[st:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}",
                        f"--input={part}", f"--output={co}"], check=True, capture_output=True)
        cos.append(co)
    return cos


def kernel_report(path, all_units=False):
    """{kernel: resources} of the first translation unit's kernels (mfgp_kernels.hip), or
    with all_units of every unit's."""
    with tempfile.TemporaryDirectory() as td:
        md, cl = [], {}
        for co in (code_objects(path, td) if all_units else [code_object(path, td)]):
            md += metadata(co)
            cl.update(calls(co))
    rep = {}
    for k in md:
        name = k[".name"]
        rep[name] = {"vgpr": k[".vgpr_count"], "agpr": k.get(".agpr_count", 0),
                     "vgpr_spill": k.get(".vgpr_spill_count", 0), "sgpr_spill": k.get(".sgpr_spill_count", 0),
                     "lds": k[".group_segment_fixed_size"], "scratch": k.get(".private_segment_fixed_size", 0),
                     "calls": cl.get(name, 0)}
    return rep


def instruction_streams(path):
    """{kernel: [(mnemonic, operands, branch target relative to the kernel's start or None)]} of
    every unit's kernels: what two builds of one source must agree on, wherever the kernels
    landed in their code objects."""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(path, td):
            for name, ins in disassembly(co).items():
                base = ins[0][0] if ins else 0
                # (a branch's operand is its target's address as text: the relative target stands for it)
                out[name] = [(op, args if t is None else "", None if t is None else t - base) for _, op, args, t in ins]
    return out


RESOURCES = ("vgpr", "agpr", "vgpr_spill", "sgpr_spill", "scratch", "lds")


def compare(old, new):
    """Two builds of the library, kernel by kernel -> {"only_old", "only_new": kernel symbols in one
    build alone; "code": kernels whose instruction streams differ; "resources": {kernel: {figure:
    (old, new)}} for the VGPR / AGPR / spill / scratch / LDS figures that differ; "kernels": the
    number compared}."""
    ro, rn = kernel_report(old, all_units=True), kernel_report(new, all_units=True)
    so, sn = instruction_streams(old), instruction_streams(new)
    both = sorted(set(ro) & set(rn))
    res = {k: {f: (ro[k][f], rn[k][f]) for f in RESOURCES if ro[k][f] != rn[k][f]} for k in both}
    return {"only_old": sorted(set(ro) - set(rn)), "only_new": sorted(set(rn) - set(ro)),
            "code": [k for k in both if so.get(k) != sn.get(k)],
            "resources": {k: v for k, v in res.items() if v}, "kernels": len(both)}


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        # usage: python tools/check_codeobj.py compare OLD.so NEW.so; exit status 1 if anything differs
        c = compare(sys.argv[2], sys.argv[3])
        for key in ("only_old", "only_new"):
            for k in c[key]:
                print(f"{key}: {k}")
        for k in c["code"]:
            print(f"code differs: {k}")
        for k, v in c["resources"].items():
            print(f"resources differ: {k}: " + ", ".join(f"{f} {a} -> {b}" for f, (a, b) in v.items()))
        same = c["kernels"] - len(set(c["code"]) | set(c["resources"]))
        print(f"{c['kernels']} kernels compared, {same} identical")
        sys.exit(1 if c["only_old"] or c["only_new"] or c["code"] or c["resources"] else 0)
    for n, r in sorted(kernel_report(sys.argv[1]).items()):
        print(n, r)
