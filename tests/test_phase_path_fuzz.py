"""Seeded fuzz of ray paths with velocities on the nasty grids of tests/test_integral_fuzz.py: trace_phase / backtrace_phase on
integral_fuzz_common.config(seed), seed in range(16), the configurations tests/test_path_fuzz.py uses (non-cubic grids of
2..24 voxels per axis, 2-voxel axes on seeds 0, 4, 7, 14, h never a power of two, steps of 0.2..1.7 cells, rough media on
seed % 3 == 0, 600 rays inside, outside and exactly on faces, at rest and off unit speed).

Referee, yardstick, compared rays, bound: tests/path_common.py::referee_phase with
integral_fuzz_common.masks(oracle, seed)["compared"] unchanged -- that set depends only on the forward march, which this
operator shares -- and MARGIN, FLOOR, CAPS and bound() of tests/integral_fuzz_common.py.  Strides 1 and 5, an M that pads and
an M that truncates, every mode of path_common.PHASE_MODES.

CPU tier: forward identities bit for bit, forward and adjoint under the bound.  GPU tier: the kernels against the host build
with and without the pair copy (the forward sorts on even seeds and the adjoint takes its order; on odd seeds the forward
runs in caller order and the adjoint sorts for itself).

Largest e_prod / max(e_ref, 2.4e-7) over the 16 seeds, host build (8 allowed): ray gradients 7.67 (seed 3, stride 1,
truncating M, dvpath on the padded entries alone, which is a seed on vt: 1.69e-4 against 2.20e-5), dL/drif 5.87 (seed 9, stride
1, truncating M, the same mode), path samples 1.16, vpath samples 1.30 (seed 6)."""
import numpy as np
import pytest

import cases
from integral_fuzz_common import SEEDS, config
import integral_fuzz_common as IF
from integral_common import ATOMIC_TOL, _same
import path_common as PC
from raygrad_common import max_steps_fwd

_bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731


# ---- CPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_forward_identities(seed):
    """(xt, vt, path, count, steps, n_failed) == trace_path's; vpath[0] == vel; padded entries == vt; the stride-5 vpath ==
    every 5th row of the stride-1 vpath; M = 3 leaves the first rows unchanged: bit for bit."""
    c = config(seed)
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    one = PC.fwd_phase(c, 1, PC.pad_m(ms, 1))
    for stride in PC.STRIDES:
        M = PC.pad_m(ms, stride)
        k = one if stride == 1 else PC.fwd_phase(c, stride, M)
        p = PC.fwd(c, stride, M)
        for key in ("xt", "vt", "path"):
            assert np.array_equal(_bits(k[key]), _bits(p[key])), key
        assert np.array_equal(k["count"], p["count"]) and np.array_equal(k["steps"], p["steps"])
        assert k["n_failed"] == p["n_failed"] > 0
        cnt = PC.count_of(k["steps"], stride, M)
        assert np.array_equal(_bits(k["vpath"][0]), _bits(c["vel"]))
        padded = np.arange(M)[:, None] >= cnt[None, :]
        assert np.array_equal(_bits(k["vpath"])[padded], _bits(np.broadcast_to(k["vt"], k["vpath"].shape))[padded])
        rows = one["vpath"][::stride][:M]
        sample = ~padded[:len(rows)]
        assert np.array_equal(_bits(k["vpath"][:len(rows)])[sample], _bits(rows)[sample])
        cut = PC.fwd_phase(c, stride, 3)
        assert np.array_equal(_bits(cut["vpath"][:min(M, 3)]), _bits(k["vpath"][:3])) and np.array_equal(cut["count"], np.minimum(cnt, 3))


@pytest.mark.parametrize("kind", ["pad", "trunc"])
@pytest.mark.parametrize("stride", PC.STRIDES)
@pytest.mark.parametrize("seed", SEEDS)
def test_referee(oracle, seed, stride, kind):
    """Forward and adjoint of the host build against float64 autograd of L = <dx, xt> + <dv, vt> + <dpath, path> +
    <dvpath, vpath> under the bound float32 autograd sets, every mode; the cap on the compared rays is
    tests/test_integral_fuzz.py's."""
    c, m = config(seed), IF.masks(oracle, seed)
    assert m["compared"].sum() >= 0.85 * 600 and m["nonzero"].sum() >= 250
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    M = PC.pad_m(ms, stride) if kind == "pad" else PC.trunc_m(ms, stride)
    worst, bad, weight = PC.referee_phase(c, m["compared"], stride, M, f"seed {seed} stride={stride} M={M}")
    assert bad == []
    # every class of seed is there; at stride 5 a configuration of few, long steps (seed 14) has no in-box sample to seed
    assert min(weight[mode] for mode in ("all", "noray", "vprefix", "vpadded")) > 0
    assert (weight["vinbox"] > 0 and weight["inbox"] > 0) or stride > 1


# ---- GPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_kernels_match_host_build(gpu, seed, pair):
    """k_trace_phase and k_backtrace_phase, plain and pair-copy gathers, stride 5, an M that pads and one that truncates ==
    the host build: both series, count, xt, vt, steps, dpos, dvel and the statistics bit for bit, the grid to the order of
    its atomic sums."""
    from adjointnonlinearraytracing_amd import drrt
    c = config(seed)
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    T = drrt.TracerC()
    fwd_sorts = seed % 2 == 0
    stride = 5
    for M in (PC.pad_m(ms, stride), PC.trunc_m(ms, stride)):
        k = PC.fwd_phase(c, stride, M)
        g, w = PC.dpath_of(k["path"].shape, seed), PC.dvpath_of(k["path"].shape, seed)
        r = PC.back_phase(c, k, c["dx"], c["dv"], g, w, stride, M, corrected_h=True)
        with drrt.using(pair_grid=pair, corrected_h=True, check_failed=False):
            with drrt.using(sort_rays=fwd_sorts):
                out, st, order = PC._gpu_forward_phase(T, c, gpu, stride, M)
            assert (order is not None) == fwd_sorts
            PC._forward_matches(out, st, k)
            with drrt.using(sort_rays=True):
                (grad, dpos, dvel), bst = PC._gpu_back_phase(T, c, gpu, out, stride, g, w, order=order)
        assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"])
        assert bst["ray_steps"] == r["ray_steps"] > 0 and bst["n_failed"] == r["n_failed"] > 0
        err = cases.rel_l2(grad.cpu().numpy(), r["grad"])
        print(f"seed {seed} pair={pair} M={M}: grid rel-L2 vs host {err:.3e}")
        assert err <= ATOMIC_TOL
