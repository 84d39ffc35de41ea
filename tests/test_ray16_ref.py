"""CPU tier of the 16-bit ray-state formats (f16, q16, qpos; include/drrt_hip.h).

* The __host__ __device__ codecs of csrc/drrt_device.h (q16_pos_enc / _dec, q16_vel_enc / _dec), compiled for the host by
  tests/hostcheck, are pinned BIT FOR BIT to the numpy restatement oracle/ray16_ref.py: every code, every code boundary,
  the range ends, the special values.  The device kernels that call them are compared with the same restatement in
  tests/test_ray16_fuzz.py.
* The seeds that GPU fuzz runs are chosen here, and what makes them worth running (a 2-voxel axis, very unequal extents,
  saturating positions, half-subnormal directions) is asserted from the oracle and the restatement alone, so a later change
  of cases.fuzz_config cannot hollow the fuzz out unnoticed.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import hostcheck_lib as H
from oracle import ray16_ref as R16
from ray16_common import ALL_I16, ALL_U16, HALF_MIN_NORMAL, SEEDS, SPECIALS, options_of, pos_sweep, reference, same_bits, vel_sweep

VOLUMES = [((256, 256, 256), 1.0 / 255), ((4, 9, 5), 0.5), ((2, 2, 2), 0.05), ((24, 2, 7), 1.9999), ((2, 25, 3), 0.0731)]
_VOL_IDS = ["x".join(map(str, r)) for r, _ in VOLUMES]


# ---- the codecs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,h", VOLUMES, ids=_VOL_IDS)
def test_parameters_match_the_restatement(res, h):
    """q_min, q_step, q_inv_step of vol_finish, and what drrt_q16_params reports, equal the restatement's to the bit."""
    from adjointnonlinearraytracing_amd import _lib
    want = np.array(R16.params(res, h), np.float32)
    assert same_bits(H.q16_params(res, h), want)
    out = (C.c_float * 3)()
    assert _lib.load().drrt_q16_params((C.c_int * 3)(*res), C.c_float(h), out) == 0
    assert same_bits(np.array(list(out), np.float32), np.array([want[0], want[1], R16.VEL_STEP], np.float32))


@pytest.mark.parametrize("res,h", VOLUMES, ids=_VOL_IDS)
def test_every_code_round_trips(res, h):
    """All 65 536 position codes and all 65 536 direction codes decode to the restatement's values, and encoding a
    decoded code returns it."""
    dec = H.q16_pos_dec(res, h, ALL_U16)
    assert same_bits(dec, R16.pos_dec(res, h, ALL_U16))
    assert np.all(np.diff(dec.astype(np.float64)) > 0), "codes must decode to strictly increasing positions"
    assert np.array_equal(H.q16_pos_enc(res, h, dec), ALL_U16)
    assert np.array_equal(R16.pos_enc(res, h, dec), ALL_U16)
    vdec = H.q16_vel_dec(res, h, ALL_I16)
    assert same_bits(vdec, R16.vel_dec(ALL_I16))
    assert np.array_equal(vdec.astype(np.float64) * 16384.0, ALL_I16.astype(np.float64))       # exact fixed point
    assert np.array_equal(H.q16_vel_enc(res, h, vdec), ALL_I16)
    assert np.array_equal(R16.vel_enc(vdec), ALL_I16)


@pytest.mark.parametrize("res,h", VOLUMES, ids=_VOL_IDS)
def test_encode_sweep_matches_the_restatement(res, h):
    x = pos_sweep(res, h)
    got, want = H.q16_pos_enc(res, h, x), R16.pos_enc(res, h, x)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (x[bad[:5]], got[bad[:5]], want[bad[:5]])
    # the sweep does what it is for: both clamps act
    assert (want == 0).sum() > 1000 and (want == 65535).sum() > 1000
    v = vel_sweep()
    got, want = H.q16_vel_enc(res, h, v), R16.vel_enc(v)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (v[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert (want == -32768).sum() > 1000 and (want == 32767).sum() > 1000


def test_direction_ties_round_to_even_and_specials_saturate():
    """Hand-checked values of the restatement itself (the direction format has exact ties: odd multiples of 2^-15)."""
    s = np.float32(2.0 ** -15)
    v = np.array([1 * s, 3 * s, 5 * s, -1 * s, -3 * s, 2.5, -2.5, np.nan, np.inf, -np.inf, 1.99997, -0.0], np.float32)
    assert R16.vel_enc(v).tolist() == [0, 2, 2, 0, -2, 32767, -32768, -32768, 32767, -32768, 32767, 0]
    res, h = (4, 9, 5), 0.5                                   # E = 4: range [-0.25, 4.25]
    x = np.array([-0.25, 4.25, -1.0, 9.0, np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32)
    assert R16.pos_enc(res, h, x).tolist() == [0, 65535, 0, 65535, 0, 65535, 0, 65535, 0]
    assert R16.half_enc(np.array([6.0e-5, 3.0e-8, 2.9e-8, 65520.0, -1e6], np.float32)).tolist() == \
        [float(np.float16(6.0e-5)), 2.0 ** -24, 0.0, np.inf, -np.inf]                 # subnormals kept, overflow to inf


def test_zero_extent_volume():
    """A 1 x 1 x 1 volume is one the marches accept (make_vol in csrc/drrt_api.hip lets exactly this one through below two
    voxels per axis), so the q16 helpers accept it too, and what they return is pinned: E = 0 gives q_min = -0, q_step = 0,
    q_inv_step = inf; every code decodes to +0; a position above zero encodes to 65535, everything else (zero of either
    sign: 0 * inf is NaN; negative; NaN) to 0."""
    from adjointnonlinearraytracing_amd import _lib
    res, h = (1, 1, 1), 0.25
    p = H.q16_params(res, h)
    assert same_bits(p, np.array([-0.0, 0.0, np.inf], np.float32)) and same_bits(p, np.array(R16.params(res, h), np.float32))
    out = (C.c_float * 3)()
    assert _lib.load().drrt_q16_params((C.c_int * 3)(*res), C.c_float(h), out) == 0
    assert same_bits(np.array(list(out), np.float32), np.array([-0.0, 0.0, 2.0 ** -14], np.float32))
    dec = H.q16_pos_dec(res, h, ALL_U16)
    assert same_bits(dec, np.zeros(65536, np.float32)) and same_bits(dec, R16.pos_dec(res, h, ALL_U16))
    x = np.concatenate([SPECIALS, np.array([1.0, -1.0, 1e-30, -1e-30], np.float32)])
    want = np.where(x > 0, 65535, 0).astype(np.uint16)
    assert np.array_equal(H.q16_pos_enc(res, h, x), want) and np.array_equal(R16.pos_enc(res, h, x), want)


# ---- the fuzz seeds -------------------------------------------------------------------------------------------------
def saturating_rays(res, h, x):
    """Per ray: does any component lie outside the q16 position range [dec(0), dec(65535)]?"""
    lo, hi = R16.pos_dec(res, h, np.array([0, 65535], np.uint16))
    x = np.asarray(x, np.float32)
    return ((x < lo) | (x > hi)).any(axis=1)


def test_seed_set_has_the_nasty_cases():
    """(a) a grid with a 2-voxel axis; (b) a grid whose extents differ by 4 x or more; (c) for q16, a seed where at least
    1 % of the input rays AND 1 % of the exit rays have a saturating position (the march starts from decoded codes, which
    are in range, so a saturating exit is a ray that marched out of the range); (d) for f16, a seed with exit-direction components that are non-zero half
    subnormals.  Also: both settings of every option that test_fuzz_against_oracle toggles occur."""
    assert 6 <= len(SEEDS) <= 10 and len(set(SEEDS)) == len(SEEDS)
    cfg = {s: cases.fuzz_config(s) for s in SEEDS}
    assert all(len(c["pos"]) == 600 for c in cfg.values())
    assert any(min(c["res"]) == 2 for c in cfg.values()), "(a)"
    ext = {s: (np.array(c["res"], np.float64) - 1) * c["h"] for s, c in cfg.items()}
    assert any(e.max() >= 4 * e.min() for e in ext.values()), "(b)"
    sat = []
    for s in SEEDS:
        r = reference("q16", s)
        a, b = saturating_rays(r["res"], r["h"], r["c"]["pos"]), saturating_rays(r["res"], r["h"], r["o"]["xt"])
        codes = r["xt"].view(np.uint16)
        assert ((codes == 0) | (codes == 65535)).any(axis=1)[b].all()
        assert not saturating_rays(r["res"], r["h"], r["wpos"]).any()       # the march starts in range: exits in `b` marched out
        sat.append((float(a.mean()), float(b.mean())))
    assert any(a >= 0.01 and b >= 0.01 for a, b in sat), ("(c)", sat)
    sub = []
    for s in SEEDS:
        v = np.abs(reference("f16", s)["vt"].astype(np.float64))
        sub.append(int(((v > 0) & (v < HALF_MIN_NORMAL)).sum()))
    assert max(sub) >= 1, ("(d)", sub)
    opts = [options_of(s) for s in SEEDS]
    assert {o["sort_rays"] for o in opts} == {True, False} and {o["pair_grid"] for o in opts} == {True, False}


def test_integer_ray_tensors_are_codes_not_numbers():
    """drrt._rays, through which every ray tensor of every call goes: int16 only where the call selects the 16-bit ray
    state, no other integer dtype anywhere, floating-point dtypes converted by value (the GPU tier makes the calls)."""
    import torch
    from adjointnonlinearraytracing_amd import drrt
    cpu = torch.device("cpu")
    codes = torch.full((4, 3), 16384, dtype=torch.int16)
    assert drrt._rays(codes, cpu, q16=True).dtype == torch.int16
    for bad, kw in ((codes, {}), (codes, dict(half=True)), (codes.int(), {}), (codes.long(), {}), (codes > 0, {}),
                    (codes.float(), dict(q16=True)), (codes.int(), dict(q16=True))):
        with pytest.raises(RuntimeError, match="16-bit ray state"):
            drrt._rays(bad, cpu, **kw)
    for ok in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        assert torch.equal(drrt._rays(torch.ones(4, 3, dtype=ok), cpu), torch.ones(4, 3))
