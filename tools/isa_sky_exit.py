"""The property behind the workgroup-uniform tile test (csrc/hip/planes.h LoadTileBytesUniform), checked on the ISA: a workgroup whose tiles are all sky leaves its kernel
before it has issued a vector-memory or LDS instruction.

Compiles the device sources that hold full-frame kernels with a tile test to gfx950 assembly (the product's flags, -S --cuda-device-only) and walks every instantiation of
those kernels in text order from its entry to the SKY EXIT: the first conditional branch behind the tile load (an s_load with a register offset -- kernel arguments are read
at immediate offsets) whose target runs into s_endpgm. On the way there may be no global_ / buffer_ / flat_ / scratch_ / ds_ instruction and no branch to a label behind the
exit other than to an end of the program. One exception, reported per kernel: the TemporalAccumulation window kernels store their flag byte (lane 0, global_store_byte) on
the exit path itself.

usage: python tools/isa_sky_exit.py [-v] [--json OUT]     exit status 1 if a kernel fails
tests/test_tile_exit.py runs check_all(); a report of the library at hand is committed as profiles/isa_sky_exit.json."""
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingdenoiser_amd import build as B  # noqa: E402

# source file -> kernels (substrings of the mangled name) whose every instantiation is checked
KERNELS = {
    "kernels_reblur_spatial.hip": ["ReblurSpatialKernel", "ReblurHitDistReconstructionKernel"],
    "kernels_reblur_ta.hip": ["ReblurTemporalAccumulationKernel"],
    "kernels_reblur_history.hip": ["ReblurHistoryFixKernel", "ReblurTemporalStabilizationKernel"],
    "kernels_relax_spatial.hip": ["RelaxHitDistReconstructionKernel", "RelaxPrePassKernel", "RelaxHistoryFixKernel", "RelaxAntiFireflyKernel"],
    "kernels_relax_ta.hip": ["RelaxTemporalAccumulationKernel", "RelaxHistoryClampingKernel"],
    "kernels_relax_atrous.hip": ["RelaxAtrousKernel"],
    "kernels_sigma.hip": ["SigmaBlurKernel", "SigmaTemporalStabilizationKernel"],
}
MEMORY = re.compile(r"^(global_|buffer_|flat_|scratch_|ds_)")
TILE_LOAD = re.compile(r"^s_load_dword(x\d+)?\s+\S+\s+s\[\d+:\d+\],\s+s\d+")  # register offset: not a kernel argument
FLAG_STORE_KERNELS = ("TemporalAccumulationKernel",)


def compile_to_asm(src, out):
    subprocess.run([B.HIPCC] + B._flags(src) + ["-S", "--cuda-device-only", "-c", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
    return out


def kernels_of(asm_path, wanted):
    """{mangled name: [(label or None, instruction text), ...]} of the wanted kernels (amdhsa kernels only)"""
    text = open(asm_path).read()
    entry = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, name = {}, None
    for line in text.split("\n"):
        s = line.split(";")[0].rstrip()
        if not s:
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            label = m.group(1)
            if not label.startswith(".L"):
                name = label if label in entry and any(w in label for w in wanted) else None
                if name:
                    out[name] = []
            elif name:
                out[name].append((label, None))
            continue
        s = s.strip()
        if name and not s.startswith("."):
            out[name].append((None, s))
        if s.startswith(".Lfunc_end"):
            name = None
    return out


def _ends_program(body, labels, label, depth=0):
    """the code at `label` runs into s_endpgm without a memory instruction (following unconditional branches)"""
    i = labels.get(label)
    while i is not None and i < len(body) and depth < 8:
        lab, ins = body[i]
        i += 1
        if ins is None:
            continue
        if ins.startswith("s_endpgm"):
            return True
        if MEMORY.match(ins) or ins.startswith("s_cbranch") or ins.startswith("s_barrier"):
            return False
        m = re.match(r"s_branch\s+(\S+)", ins)
        if m:
            return _ends_program(body, labels, m.group(1), depth + 1)
    return False


def check_kernel(name, body):
    labels = {lab: i for i, (lab, ins) in enumerate(body) if lab}
    seen_tile_load, memory, stores, exit_at = False, [], 0, None
    for i, (lab, ins) in enumerate(body):
        if ins is None:
            continue
        if TILE_LOAD.match(ins):
            seen_tile_load = True
        if MEMORY.match(ins):
            if ins.startswith("global_store_byte") and any(k in name for k in FLAG_STORE_KERNELS):
                stores += 1
            else:
                memory.append(ins)
        m = re.match(r"s_cbranch_\w+\s+(\S+)", ins)
        if m and seen_tile_load and _ends_program(body, labels, m.group(1)):
            exit_at = i
            break
        if ins.startswith("s_endpgm") and seen_tile_load:
            exit_at = i
            break
    escapes = []
    if exit_at is not None:
        for lab, ins in body[:exit_at]:
            m = ins and re.match(r"s_c?branch\w*\s+(\S+)", ins)
            if m and labels.get(m.group(1), -1) > exit_at and not _ends_program(body, labels, m.group(1)):
                escapes.append(ins)
    ok = exit_at is not None and not memory and not escapes and stores <= 1
    return {"ok": ok, "instructions_to_exit": None if exit_at is None else sum(1 for _, ins in body[: exit_at + 1] if ins), "memory_before_exit": memory[:4],
            "branches_past_exit": escapes[:4], "flag_byte_stores_on_exit_path": stores, "exit_found": exit_at is not None}


def check_all(verbose=False):
    tmp = tempfile.mkdtemp(prefix="nrd_isa_")
    srcs = [(os.path.join(B.CSRC, "hip", f), os.path.join(tmp, f + ".s"), wanted) for f, wanted in KERNELS.items()]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda s: compile_to_asm(s[0], s[1]), srcs))
    report = {}
    for src, asm, wanted in srcs:
        for name, body in kernels_of(asm, wanted).items():
            report[name] = check_kernel(name, body)
        os.remove(asm)
    os.rmdir(tmp)
    if verbose:
        bad = [k for k, v in report.items() if not v["ok"]]
        print("%d kernels checked, %d without a clean sky exit" % (len(report), len(bad)))
        for k in bad:
            print("  ", k, report[k])
    return report


def main():
    report = check_all(verbose=True)
    if "--json" in sys.argv:
        digest_file = B.product_path() + ".digest"
        families = {}
        for k, v in report.items():
            fam = next(w for ws in KERNELS.values() for w in ws if w in k)
            f = families.setdefault(fam, {"instantiations": 0, "failed": 0, "instructions_to_exit_min": None, "instructions_to_exit_max": None, "flag_byte_stores_on_exit_path_max": 0})
            f["instantiations"] += 1
            f["failed"] += 0 if v["ok"] else 1
            n = v["instructions_to_exit"]
            if n is not None:
                f["instructions_to_exit_min"] = n if f["instructions_to_exit_min"] is None else min(n, f["instructions_to_exit_min"])
                f["instructions_to_exit_max"] = n if f["instructions_to_exit_max"] is None else max(n, f["instructions_to_exit_max"])
            f["flag_byte_stores_on_exit_path_max"] = max(f["flag_byte_stores_on_exit_path_max"], v["flag_byte_stores_on_exit_path"])
        summary = {"what": "tools/isa_sky_exit.py: instructions from the kernel entry to the workgroup-uniform sky exit, none of them vector-memory or LDS (the flag-byte store of the "
                           "TemporalAccumulation window kernels excepted)",
                   "library_digest": open(digest_file).read().strip() if os.path.exists(digest_file) else None, "kernels": len(report),
                   "failed": sorted(k for k, v in report.items() if not v["ok"]), "families": families}
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fp:
            json.dump(summary, fp, indent=1)
            fp.write("\n")
    sys.exit(0 if report and all(v["ok"] for v in report.values()) else 1)


if __name__ == "__main__":
    main()
