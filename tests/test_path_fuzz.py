"""Seeded fuzz of the ray-path operator on the nasty grids of tests/test_integral_fuzz.py: trace_path / backtrace_path on
cases.fuzz_config(seed), seed in range(16) (non-cubic grids of 2..24 voxels per axis, 2-voxel axes on seeds 0, 4, 7, 14, h
never a power of two, steps of 0.2..1.7 cells, rough media on seed % 3 == 0, 600 rays inside, outside and exactly on faces, at
rest and off unit speed).

Referee, yardstick, compared rays, bound: tests/path_common.py::referee with integral_fuzz_common.masks(oracle, seed)["compared"]
unchanged -- that set depends only on the forward march, which this operator shares -- and MARGIN, FLOOR, CAPS and bound() of
tests/integral_fuzz_common.py.  Strides 1 and 5, an M that pads and an M that truncates, every mode of path_common.PATH_MODES.

CPU tier: forward identities bit for bit, forward and adjoint under the bound.  GPU tier: the kernels against the host build
with and without the pair copy (the forward sorts on even seeds and the adjoint takes its order; on odd seeds the forward
runs in caller order and the adjoint sorts for itself).

Largest e_prod / max(e_ref, 2.4e-7) over the 16 seeds, host build (8 allowed): ray gradients 4.27 (seed 6, stride 5, padded
seeds alone: 1.18e-4 against 2.77e-5), dL/drif 4.73 (seed 9, stride 1, truncating M, in-box seeds alone), path samples 1.16."""
import numpy as np
import pytest

import cases
import hostcheck_lib as HC
from integral_fuzz_common import SEEDS, config
import integral_fuzz_common as IF
from integral_common import ATOMIC_TOL, _same
import path_common as PC
from raygrad_common import max_steps_fwd

_bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731


# ---- CPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_forward_identities(seed):
    """(xt, vt, steps, n_failed) == hostcheck_lib.trace; path[0] == pos; padded entries == xt; count == the formula; the
    stride-5 path == every 5th row of the stride-1 path: bit for bit."""
    c = config(seed)
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    t = HC.trace(c["rif"], c["res"], c["pos"], c["vel"], c["h"], c["ds"])
    one = PC.fwd(c, 1, PC.pad_m(ms, 1))
    for stride in PC.STRIDES:
        M = PC.pad_m(ms, stride)
        k = one if stride == 1 else PC.fwd(c, stride, M)
        assert np.array_equal(_bits(k["xt"]), _bits(t["xt"])) and np.array_equal(_bits(k["vt"]), _bits(t["vt"]))
        assert np.array_equal(k["steps"].astype(np.int64), t["steps"].astype(np.int64)) and k["n_failed"] == t["n_failed"] > 0
        cnt = PC.count_of(k["steps"], stride, M)
        assert np.array_equal(k["count"], cnt) and np.array_equal(_bits(k["path"][0]), _bits(c["pos"]))
        padded = np.arange(M)[:, None] >= cnt[None, :]
        assert np.array_equal(_bits(k["path"])[padded], _bits(np.broadcast_to(k["xt"], k["path"].shape))[padded])
        rows = one["path"][::stride][:M]
        sample = ~padded[:len(rows)]
        assert np.array_equal(_bits(k["path"][:len(rows)])[sample], _bits(rows)[sample])
        cut = PC.fwd(c, stride, 3)
        assert np.array_equal(_bits(cut["path"][:min(M, 3)]), _bits(k["path"][:3])) and np.array_equal(cut["count"], np.minimum(cnt, 3))


@pytest.mark.parametrize("kind", ["pad", "trunc"])
@pytest.mark.parametrize("stride", PC.STRIDES)
@pytest.mark.parametrize("seed", SEEDS)
def test_referee(oracle, seed, stride, kind):
    """Forward and adjoint of the host build against float64 autograd of L = <dx, xt> + <dv, vt> + <dpath, path> under the
    bound float32 autograd sets, every mode; the cap on the compared rays is tests/test_integral_fuzz.py's."""
    c, m = config(seed), IF.masks(oracle, seed)
    assert m["compared"].sum() >= 0.85 * 600 and m["nonzero"].sum() >= 250
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    M = PC.pad_m(ms, stride) if kind == "pad" else PC.trunc_m(ms, stride)
    worst, bad, weight = PC.referee(c, m["compared"], stride, M, f"seed {seed} stride={stride} M={M}")
    assert bad == []
    # every class of seed is there; at stride 5 a configuration of few, long steps (seed 14) has no in-box sample to seed
    assert min(weight[mode] for mode in ("all", "noray", "prefix", "padded")) > 0 and (weight["inbox"] > 0 or stride > 1)


# ---- GPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_kernels_match_host_build(gpu, seed, pair):
    """k_trace_path and k_backtrace_path, plain and pair-copy gathers, stride 5, an M that pads and one that truncates == the
    host build: path, count, xt, vt, steps, dpos, dvel and the statistics bit for bit, the grid to the order of its atomic
    sums."""
    from adjointnonlinearraytracing_amd import drrt
    c = config(seed)
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    T = drrt.TracerC()
    fwd_sorts = seed % 2 == 0
    stride = 5
    for M in (PC.pad_m(ms, stride), PC.trunc_m(ms, stride)):
        k = PC.fwd(c, stride, M)
        g = PC.dpath_of(k["path"].shape, seed)
        r = PC.back(c, k, c["dx"], c["dv"], g, stride, M, corrected_h=True)
        with drrt.using(pair_grid=pair, corrected_h=True, check_failed=False):
            with drrt.using(sort_rays=fwd_sorts):
                out, st, order = PC._gpu_forward(T, c, gpu, stride, M)
            assert (order is not None) == fwd_sorts
            PC._forward_matches(out, st, k)
            with drrt.using(sort_rays=True):
                (grad, dpos, dvel), bst = PC._gpu_back(T, c, gpu, out, stride, g, order=order)
        assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"])
        assert bst["ray_steps"] == r["ray_steps"] > 0 and bst["n_failed"] == r["n_failed"] > 0
        err = cases.rel_l2(grad.cpu().numpy(), r["grad"])
        print(f"seed {seed} pair={pair} M={M}: grid rel-L2 vs host {err:.3e}")
        assert err <= ATOMIC_TOL
