"""What the 16-bit ray-state and sort-order test files (test_ray16_ref.py, test_ray16_fuzz.py, test_sort_order.py,
test_sortkey_ref.py) share: the fuzz seeds and modes, the sweeps of the two encoders, the reference of a (mode, seed) and the
float64 referee of the sort keys.  A plain module: no fixtures, no tests."""
import functools

import numpy as np

import cases
from oracle import ray16_ref as R16
from oracle import sortkey_ref as S

ALL_U16 = np.arange(65536, dtype=np.uint16)
ALL_I16 = np.arange(-32768, 32768, dtype=np.int16)

# fp32 values every sweep contains: signed zeros, the smallest and the largest denormal, the smallest normal, huge, infinite, NaN
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38,
                     3e38, -3e38, np.inf, -np.inf, np.nan], np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[np.asarray(a).dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _around(v):
    """v, one ulp below and one ulp above (fp32)."""
    v = np.asarray(v, np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])


def pos_sweep(res, h, seed=0):
    """Positions at which a wrong rounding, clamp or parameter of the position encoder shows: every code's value and the
    midpoint to the next code (each +- 0, 1 ulp), both range ends and one step beyond, the specials, 200 000 seeded
    uniform values over 1.5 x the range."""
    q_min, q_step, _ = R16.params(res, h)
    dec = R16.pos_dec(res, h, ALL_U16)
    mid = ((dec[:-1].astype(np.float64) + dec[1:].astype(np.float64)) / 2).astype(np.float32)
    ends = np.array([dec[0], dec[-1], dec[0] - q_step, dec[-1] + q_step], np.float32)
    lo, hi = float(dec[0]), float(dec[-1])
    rng = np.random.default_rng(16 + seed)
    uni = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), 200_000).astype(np.float32)
    return np.concatenate([_around(dec), _around(mid), _around(ends), SPECIALS, uni])


def vel_sweep(seed=0):
    """The same for the direction encoder (range [-2, 2 - 2^-14], step 2^-14)."""
    dec = R16.vel_dec(ALL_I16)
    mid = (dec[:-1] + dec[1:]) / np.float32(2)                  # exact: multiples of 2^-15
    ends = np.array([dec[0], dec[-1], dec[0] - R16.VEL_STEP, dec[-1] + R16.VEL_STEP], np.float32)
    rng = np.random.default_rng(61 + seed)
    uni = rng.uniform(-3.0, 3.0, 200_000).astype(np.float32)
    return np.concatenate([_around(dec), _around(mid), _around(ends), SPECIALS, uni])

MODES = R16.MODES
SEEDS = (0, 1, 3, 5, 7, 8, 44, 61)          # chosen by scanning seeds 0..63 for the properties asserted below
HALF_MIN_NORMAL = 2.0 ** -14                 # 6.1e-5: below it an IEEE half is subnormal


def options_of(seed):
    """Library options of a seed, as tests/test_gpu_fuzz.py::test_fuzz_against_oracle toggles them."""
    return dict(sort_rays=bool(seed % 2), pair_grid=(seed % 4 == 1))


@functools.lru_cache(maxsize=None)
def reference(mode, seed):
    """Everything a test of (mode, seed) compares with, computed once from cases.fuzz_config, the restatement and the
    factored-arithmetic oracle -- never from the library: the stored inputs (`pos`, `vel`, `dx`, `dv`), their widened
    values (`w*`), the oracle's forward march of the widened inputs (`o`), its exit rays as the library must store them
    (`xt`, `vt`) and widened again (`wxt`, `wvt`).  Callers must not modify it."""
    from oracle import oracle as O
    O.build()
    c = cases.fuzz_config(seed)
    res, h, ds = c["res"], c["h"], c["ds"]
    r = dict(c=c, res=res, h=h, ds=ds)
    for name, kind, src in (("pos", "pos", "pos"), ("vel", "vel", "vel"), ("dx", "seed", "dx"), ("dv", "seed", "dv")):
        r[name] = R16.store(mode, kind, c[src], res, h)
        r["w" + name] = R16.widen(mode, kind, r[name], res, h)
    with O.arith("factored"):
        r["o"] = O.trace(c["rif"], res, r["wpos"], r["wvel"], h, ds, dtype=np.float32)
    r["xt"], r["vt"] = R16.store(mode, "pos", r["o"]["xt"], res, h), R16.store(mode, "vel", r["o"]["vt"], res, h)
    r["wxt"], r["wvt"] = R16.widen(mode, "pos", r["xt"], res, h), R16.widen(mode, "vel", r["vt"], res, h)
    return r


def referee(res, h, pos, vel, sign, chord):
    """-> (float64 keys, decided)"""
    if chord:
        r = S.chord64(res, h, pos, vel, sign, hit32=S.chord32(res, h, pos, vel, sign)["hit"])
    else:
        r = S.lightfield64(res, h, pos, vel, sign)
    return r["key"], r["decided"]
