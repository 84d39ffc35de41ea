#!/usr/bin/env python3
"""python tools/isa_diff.py BASE_REV : compare the gfx950 machine code of the library's kernels between BASE_REV and
the working tree.

Every unit of the library is compiled with the Makefile's own commands (``make -n``: its CXXFLAGS, and RINGFLAGS for
the ring-window unit) with ``-c`` replaced by ``--cuda-device-only -S``, once from ``git archive BASE_REV`` and once
from the working tree.  The bodies of k_backtrace_flat, k_backtrace_ring, k_backtrace_direct, k_backtrace_rays,
k_backtrace_opl, k_backtrace_field, k_backtrace_emission, k_backtrace_vector, k_backtrace_path, k_backtrace_phase (k_trace_opl, k_trace_field, k_trace_emission, k_trace_vector, k_trace_path and k_trace_phase come with k_trace*), k_backtrace_cable*, k_backtrace_stop_rays*, k_backtrace_target_rays, k_target_* (the forward target march and the count pass
of its ray-state adjoint), k_bundle_classify, k_trace*, the utility kernels of drrt_api.hip (k_build_pair,
k_q16_*, k_chunk_progress_init), the sort-key kernels (k_lightfield_keys, k_chord_keys) and the operator kernels around the march (k_sensor_*, k_gen_*, k_upres, k_adam_masked,
k_rays_to_plane*) are compared instantiation by instantiation, with the label numbers (which depend on a function's
position in its unit) normalised and comments dropped.  A kernel is matched by its demangled name, so one that moved to
another unit is still compared.  Prints one line per instantiation and exits 1 if any present on both sides differs.
"""
import os
import re
import subprocess
import sys
import tempfile

KERNELS = ("k_backtrace_flat", "k_backtrace_ring", "k_backtrace_direct", "k_backtrace_rays", "k_backtrace_opl", "k_backtrace_field", "k_backtrace_emission", "k_backtrace_vector", "k_backtrace_path", "k_backtrace_phase", "k_backtrace_cable",
           "k_backtrace_stop_rays", "k_backtrace_target_rays", "k_target_", "k_bundle_classify", "k_trace", "k_build_pair", "k_q16_", "k_chunk_progress_init",
           "k_sensor_", "k_gen_", "k_upres", "k_adam_masked", "k_rays_to_plane", "k_lightfield_keys", "k_chord_keys")
CSRC = "adjointnonlinearraytracing_amd/csrc"
FILT = "c++filt"


def compile_units(csrc, out):
    """Device assembly of every unit, by the Makefile's compile commands -> {unit: path of its .s}"""
    dry = subprocess.run(["make", "-s", "-n", "-B", "-C", csrc], capture_output=True, text=True, check=True).stdout
    procs = {}
    for line in dry.splitlines():
        m = re.search(r" -c (\S+)\.hip -o \S+$", line)
        if not m:
            continue
        unit = m.group(1)
        asm = os.path.join(out, unit + ".s")
        cmd = line[:m.start()] + f" --cuda-device-only -S {unit}.hip -o {asm}"
        procs[unit] = (asm, subprocess.Popen(cmd, shell=True, cwd=csrc))
    for unit, (_, p) in procs.items():
        if p.wait() != 0:
            sys.exit(f"isa_diff: compiling {unit} in {csrc} failed")
    return {u: a for u, (a, _) in procs.items()}


def kernel_bodies(asm_path):
    """{demangled name: normalised body} of the kernels of interest in one assembly file"""
    lines = open(asm_path).read().splitlines()
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"(_Z\w+):", l)] if m]
    names = subprocess.run([FILT], input="\n".join(s for _, s in starts), capture_output=True, text=True,
                           check=True).stdout.splitlines()
    bodies = {}
    for (i, sym), name in zip(starts, names):
        if not any(k in name for k in KERNELS):
            continue
        body = []
        for l in lines[i + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";", 1)[0].rstrip()
            if l:
                body.append(re.sub(r"\.(LBB|Ltmp|LBB_END)\d+_", r".\1_", re.sub(r"\.Ltmp\d+", ".Ltmp", l)))
        bodies[name] = body
    return bodies


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = subprocess.run(["git", "rev-parse", "--show-toplevel"], capture_output=True, text=True,
                          check=True).stdout.strip()
    with tempfile.TemporaryDirectory() as tmp:
        base_tree = os.path.join(tmp, "base")
        os.makedirs(base_tree)
        arch = subprocess.run(["git", "-C", root, "archive", sys.argv[1]], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", base_tree], input=arch, check=True)
        sides = {}
        for side, tree in (("base", base_tree), ("head", root)):
            out = os.path.join(tmp, side + "_s")
            os.makedirs(out)
            sides[side] = {}
            for asm in compile_units(os.path.join(tree, CSRC), out).values():
                sides[side].update(kernel_bodies(asm))
    base, head = sides["base"], sides["head"]
    differ = 0
    for name in sorted(set(base) | set(head)):
        if name not in head:
            status = "removed"
        elif name not in base:
            status = "added"
        elif base[name] == head[name]:
            status = f"identical ({len(head[name])} lines)"
        else:
            status = "DIFFERS"
            differ += 1
        print(f"{status:24s} {name}")
    print(f"{len(base)} kernels at {sys.argv[1]}, {len(head)} in the working tree, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
