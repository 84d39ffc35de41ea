"""Radiance splats: sensor.splat_radiance / splat_radiance_far (csrc/drrt_sensor.hip k_sensor_radiance,
k_sensor_radiance_bwd) -- a per-ray, per-channel energy onto a (C, res, res) image, with gradients for the rays AND the
energy.

CPU tier: the fixture tests/golden/sensor_radiance.npz (the reference's generate_sensor / generate_inf_sensor run per
channel, torch.autograd for dL/de, dL/dx, dL/dv) against the float64 restatements; the eight C entries declared, exported,
bound and refusing bad calls before any HIP call; the Python operators' refusals.

GPU tier: the fixture reproduced; a seeded fuzz against the restatements on fp32-rounded inputs under the per-element
error model of tests/test_sensor_fuzz.py,  |kernel - restatement| <= c 2^-24 S  with S the sum of the magnitudes of the
output's terms (the effect of the rounding of the sensor coordinate u included), from whose helpers the model is built;
exact facts (misses, channel independence, outputs asked for alone); agreement with generate_sensor; the call path.

dL/drad = F0 G_c (F0 = |v.n|, far field 1):  S = F0 x terms of G_c + |G_c| x terms of v.n + F0 |dG_c/du| x terms of u.  G is
continuous in u (a tap enters or leaves with weight 0), so EVERY ray is compared for dL/drad; the ray gradients keep the
KINK exclusion of tests/test_sensor_fuzz.py and its cap, asserted on the restatement's own taps before anything is
compared."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cases
import sensor_radiance_common as R
from sensor_radiance_common import KINK, KINK_FRACTION
from oracle import sensor_ref as S
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# c of each bound; after each, the largest err / (2^-24 S) measured on an MI355X over the cases below
# (twice the measured value, rounded up to the next 0.5; a measured ratio above 4 would mean that the terms are wrong)
C_RAD_IMG, C_RAD_E, C_RAD_G = 1.0, 1.5, 1.0                  # near: image per pixel [0.45], dL/drad [0.57], ray gradients [0.25]
C_RADFAR_IMG, C_RADFAR_E, C_RADFAR_G = 1.0, 1.5, 0.5         # far: image per pixel [0.48], dL/drad [0.65], dL/dv [0.07]


# ---- CPU tier --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["near", "far"])
def test_fixture_matches_the_restatements(tag):
    """The reference run (float64) against oracle/sensor_ref.py per channel, its *_backward summed over the channels, and
    the new restatement of dL/drad."""
    c = R.fixture(tag)
    args = (c["x"], c["v"], c["rad"], c["p"], c["n"], c["res"], c["arg"])
    assert c["rad"].shape == (1024, 3) and c["img"].shape == (3, 24, 24)
    img = R.images(*args, c["t"], c["far"])
    assert np.abs(img - c["img"]).max() <= 1e-12 * np.abs(c["img"]).max()
    gx, gv = R.ray_grads(*args, c["gI"], c["t"], c["far"])
    for got, key in ((gx, "gx"), (gv, "gv")):
        assert np.abs(got - c[key]).max() <= 1e-10 * max(np.abs(c[key]).max(), 1e-300), key     # far: gx is 0 on both sides
    ge = R.grad_rad(c["x"], c["v"], c["p"], c["n"], c["res"], c["arg"], c["gI"], c["t"], c["far"])
    assert np.abs(ge - c["ge"]).max() <= 1e-10 * np.abs(c["ge"]).max()
    # what the fixture is meant to hold
    miss = (c["ge"] == 0).all(1)
    assert 0.15 <= miss.mean() <= 0.4 and (c["rad"] < 0).any() and (c["rad"] == 0).any()
    if not c["far"]:
        den = c["v"] @ c["n"]
        assert (den < 0).any() and (den > 0).any() and ((((c["p"] - c["x"]) @ c["n"]) / den) < 0).any()
    assert os.path.getsize(R.GOLDEN) <= 256 * 1024


@pytest.fixture(scope="module")
def lib():
    from adjointnonlinearraytracing_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "adjointnonlinearraytracing_amd", "csrc")], check=True)
    return _lib


_ENTRIES = {f"drrt_sensor_radiance{far}{d}{b}_f32":
            f"n {'v' if far else 'x v'} rad channels {'frame12' if d else ('t1 t2' if far else 'plane_p plane_n t1 t2')} "
            f"res span {'grad_image grad_rad grad_x grad_v' if b else 'image flags'} stream"
            for far in ("", "_far") for d in ("", "_dframe") for b in ("", "_bwd")}
_HOST_VEC3 = ("plane_p", "plane_n", "t1", "t2")


def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "drrt_hip.h")).read()
    declared = set(re.findall(r"DRRT_API\s+int\s+(drrt_sensor_radiance\w+)\s*\(", header))
    assert declared == set(_ENTRIES) and len(declared) == 8
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert declared <= set(re.findall(r"\bT (drrt_\w+)", out))
    assert declared <= set(lib.SIGNATURES) and declared == set(lib._radiance_signatures())
    h = lib.load()
    for e, names in _ENTRIES.items():
        assert len(getattr(h, e).argtypes) == len(names.split()), e
    for e, names in _ENTRIES.items():                 # the header's argument names, in order
        m = re.search(r"DRRT_API\s+int\s+" + e + r"\s*\(([^;]*)\);", header)
        assert [re.findall(r"\w+", a.split("[")[0])[-1] for a in m.group(1).split(",")] == \
            names.replace("span", "ang_cut" if "_far" in e else "span").split(), e


_NULL, _SPAN, _CH = (-3, "null pointer"), (-3, "bad sensor resolution / span"), (-3, "channels must lie in 1..32")
_ROWS = [       # (row, overrides, answer): refused -- or DRRT_OK for nothing to do -- before the first HIP call
    ("null_x", dict(x=None, res=0), _NULL), ("null_v", dict(v=None, span=0.0), _NULL), ("null_t1", dict(t1=None, res=0), _NULL),
    ("null_plane_n", dict(plane_n=None), _NULL),
    ("null_frame12", dict(frame12=None, v=None), (-3, "null frame pointer")),
    ("res0", dict(res=0, rad=None), _SPAN), ("res32769", dict(res=32769, channels=0), _SPAN), ("span0", dict(span=0.0), _SPAN),
    ("span_nan", dict(span=float("nan"), n=0), _SPAN), ("span_neg", dict(span=-1.0), _SPAN),
    ("null_rad", dict(rad=None, channels=0), _NULL),
    ("channels0", dict(channels=0, image=None, grad_image=None), _CH), ("channels33", dict(channels=33, n=0), _CH),
    ("channels_neg", dict(channels=-1), _CH),
    ("null_image", dict(image=None, n=0), (-3, "null image pointer")),
    ("null_grad_image", dict(grad_image=None, n=0, grad_rad=None, grad_x=None, grad_v=None), (-3, "null gradient pointer")),
    ("ok_no_outputs", dict(grad_rad=None, grad_x=None, grad_v=None), 0),            # n = 128: nothing is launched
    ("ok_n0", dict(n=0), 0), ("ok_n0_32_channels", dict(n=0, channels=32), 0),      # (flags: DRRT_FLAG_NO_ZERO, no fill)
]


def _invoke(h, entry, overrides):
    vals = dict(n=128, channels=3, res=8, span=1.0, flags=4, stream=None)
    args = []
    for k in _ENTRIES[entry].split():
        v = overrides[k] if k in overrides else vals.get(k, 0x1000)       # 0x1000: a non-null pointer, never dereferenced
        args.append((C.c_float * 3)(0.0, 1.0, 0.0) if k in _HOST_VEC3 and v is not None else v)
    return getattr(h, entry)(*args)


def test_bad_calls_are_refused_before_any_hip_call(lib):
    """As tests/test_abi.py::test_operator_calls_are_answered_by_the_same_check for the existing families: code and
    message of every refusal, and DRRT_OK without a launch where there is nothing to do.  Runs without a GPU; rows with
    two faults pin which check answers (frame, pointers, resolution / span, rad, channels, outputs)."""
    h = lib.load()
    seen = set()
    for entry, names in _ENTRIES.items():
        for row, overrides, want in _ROWS:
            given = {k: v for k, v in overrides.items() if k in names.split()}
            lead = next(iter(overrides))
            if lead not in given:
                continue
            rc = _invoke(h, entry, given)
            got = 0 if rc == 0 else (rc, h.drrt_last_error().decode())
            assert got == want, (entry, row)
            seen.add((row, entry))
    assert {r for r, _ in seen} == {r for r, _, _ in _ROWS}
    for row in ("null_v", "res0", "null_rad", "channels0", "channels33", "ok_n0"):
        assert sum(r == row for r, _ in seen) == 8, row
    assert sum(r == "ok_no_outputs" for r, _ in seen) == sum(r == "null_grad_image" for r, _ in seen) == 4


def _cpu_call(op, **over):
    from adjointnonlinearraytracing_amd import sensor
    N = 8
    ins = dict(rad=torch.rand(N, 3), p=torch.tensor([[0.5, 1.2, 0.5]]), n=torch.tensor([[0.0, 1.0, 0.0]]),
               tangent=torch.tensor([[0.0, 0.0, 1.0]]))
    ins.update(over)
    fn = sensor.splat_radiance if op == "near" else sensor.splat_radiance_far
    return fn((torch.rand(N, 3), torch.rand(N, 3)), ins["rad"], (ins["p"], ins["n"]), 16, 1.0 if op == "near" else 120,
              tangent=ins["tangent"])


@pytest.mark.parametrize("op,arg", [("near", "p"), ("near", "n"), ("near", "tangent"), ("far", "n"), ("far", "tangent")])
def test_planes_that_require_grad_are_refused(op, arg):
    """Plane gradients stay out of scope: the refusal of generate_sensor, in the same words."""
    t = dict(p=torch.tensor([[0.5, 1.2, 0.5]]), n=torch.tensor([[0.0, 1.0, 0.0]]), tangent=torch.tensor([[0.0, 0.0, 1.0]]))[arg]
    with pytest.raises(RuntimeError, match=f"w.r.t. `{arg}`.*{arg}.detach"):
        _cpu_call(op, **{arg: t.requires_grad_(True)})


@pytest.mark.parametrize("op", ["near", "far"])
def test_rad_of_the_wrong_kind_is_refused(op):
    for rad in (1.0, torch.tensor(1.0)):
        with pytest.raises(RuntimeError, match="generate_sensor"):
            _cpu_call(op, rad=rad)
    for shape in ((9,), (8, 0), (8, 33), (8, 2, 2)):
        with pytest.raises(RuntimeError, match="`rad` must have"):
            _cpu_call(op, rad=torch.rand(*shape))
    with pytest.raises(RuntimeError, match="no CPU path"):         # a good call on CPU tensors gets as far as the device check
        _cpu_call(op, rad=torch.rand(8, 32, requires_grad=True))


# ---- GPU tier --------------------------------------------------------------------------------------------------------
def _run(gpu, far, x, v, rad, p, n, t2, res, arg, gI):
    """Both frame paths -> [(image, dL/drad, dL/dx, dL/dv)] x 2, the per-ray outputs equal."""
    from adjointnonlinearraytracing_amd import sensor
    fn = sensor.splat_radiance_far if far else sensor.splat_radiance

    def run(P, N, T):
        xs, vs, rs = (R.to_dev(a, gpu).requires_grad_(True) for a in (x, v, rad))
        img = fn((xs, vs), rs, (P, N), res, arg, T)
        (img * R.to_dev(gI, gpu)).sum().backward()
        assert not far or xs.grad is None or not xs.grad.any()          # the positions do not enter the far field
        return R.to_np(img), R.to_np(rs.grad), np.zeros(x.shape) if xs.grad is None else R.to_np(xs.grad), R.to_np(vs.grad)

    outs = R.both_frames(gpu, run, p, n, t2)
    R.same_per_ray([o[1:] for o in outs], ("dL/drad", "dL/dx", "dL/dv"))
    return outs


def _model(x, v, rad, p, n, t2, t1, res, arg, far, gI):
    """The restatement's outputs and the terms S of each -> dict."""
    c = R.coords(x, v, p, n, arg, t2, far)
    taps = S._taps(c["xn"], res, c["span"])
    hs = taps[0]
    u = c["xn"] / hs - 0.5
    F0 = c["F0"]
    if far:
        nv = np.linalg.norm(v, axis=-1, keepdims=True)
        vh = v / nv
        U = R.u_terms(3 * (np.abs(vh) @ (np.abs(t1) + np.abs(t2))), c["span"] / 2, hs, u)
        F0_terms = np.zeros(len(v))
    else:
        den, t, dt = R.plane_terms(x, v, p, n)
        U = R.u_terms(R.near_qt(x, v, p, t, dt, t1, t2), c["span"] / 2, hs, u)
        F0_terms = np.abs(v * n).sum(-1)
    nc = rad.shape[1]
    m = dict(img=R.images(x, v, rad, p, n, res, arg, t2, far), ge=R.grad_rad(x, v, p, n, res, arg, gI, t2, far),
             img_terms=np.zeros((nc, res, res)), ge_terms=np.zeros(rad.shape), taps=taps, U=U)
    m["gx"], m["gv"] = R.ray_grads(x, v, rad, p, n, res, arg, gI, t2, far)
    gq, mq, fore = np.zeros((len(v), 3)), np.zeros((len(v), 3)), np.zeros(len(v))
    for k in range(nc):
        G, Gu, A0, A1, H, kink = R.tent(taps, R.seed_taps(taps, gI[k], res))
        m["ge_terms"][:, k] = F0 * A0 + np.abs(G) * F0_terms + F0 * np.abs(Gu).sum(-1) * U
        Fk = F0 * rad[:, k]
        m["img_terms"][k] = R.image_terms(taps, Fk, U, res)
        a, b = R.grad_chain(Fk[:, None] * Gu, (np.abs(Fk) * (A1 + H * U))[:, None], hs, t1, t2)
        gq += a; mq += b
        fore += np.abs(rad[:, k]) * (np.abs(G) + A0 + np.abs(Gu).sum(-1) * U)
    if far:
        m["gx_terms"] = np.zeros((len(v), 3))
        m["gv_terms"] = (mq + np.abs(vh) * ((np.abs(vh) * mq).sum(-1) + np.abs(vh * gq).sum(-1))[:, None]) / nv + 4 * np.abs(m["gv"])
    else:
        m["gx_terms"], m["gv_terms"] = R.plane_chain(gq, mq, v, n, den, t, dt)
        m["gv_terms"] = m["gv_terms"] + fore[:, None] * np.abs(n)
    m["keep"] = kink > KINK * np.maximum(U, 1.0)            # (the taps' distances are the same for every channel)
    m["no_tap"] = ~taps[7].any(axis=(1, 2))                 # rays without a tap on the image
    return m


def _compare(name, outs, m, far):
    ci, ce, cg = (C_RADFAR_IMG, C_RADFAR_E, C_RADFAR_G) if far else (C_RAD_IMG, C_RAD_E, C_RAD_G)
    left_out = float((~m["keep"]).mean())
    print(f"\n[radiance fuzz] {name}: {left_out:.2%} of the rays near a kink")
    assert left_out <= KINK_FRACTION
    for k, o in enumerate(outs):
        R.check(f"{name} image ({'host' if k == 0 else 'device'} frame)", o[0], m["img"], m["img_terms"], ci)
    _, ge, gx, gv = outs[0]
    R.check(f"{name} dL/drad", ge, m["ge"], m["ge_terms"], ce)                       # every ray
    R.check(f"{name} dL/dx", gx, m["gx"], m["gx_terms"], cg, m["keep"])
    R.check(f"{name} dL/dv", gv, m["gv"], m["gv_terms"], cg, m["keep"])
    for a, what in ((ge, "dL/drad"), (gx, "dL/dx"), (gv, "dL/dv")):
        assert not a[m["no_tap"]].any(), f"{name}: {what} of a ray that misses is not exactly 0"


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["near", "far"])
def test_fixture_is_reproduced(gpu, tag):
    """The reference run: image, dL/dx, dL/dv within the bounds tests/test_sensor.py puts on generate_sensor's and
    generate_inf_sensor's reference-run fixtures (rel-L2 2e-6 / 2e-4 near, 5e-6 / 3e-4 far), dL/drad within the error
    model; both frame paths."""
    c = R.fixture(tag)
    far = c["far"]
    t1 = np.cross(c["n"], c["t"])
    outs = _run(gpu, far, c["x"], c["v"], c["rad"], c["p"], c["n"], c["t"], c["res"], c["arg"], c["gI"])
    m = _model(c["x"], c["v"], c["rad"], c["p"], c["n"], c["t"], t1, c["res"], c["arg"], far, c["gI"])
    for img, ge, gx, gv in outs:
        assert img.shape == (3, c["res"], c["res"])
        assert cases.rel_l2(img, c["img"]) <= (5e-6 if far else 2e-6)
        assert cases.rel_l2(gv, c["gv"]) <= (3e-4 if far else 2e-4)
        if far:
            assert not gx.any()
        else:
            assert cases.rel_l2(gx, c["gx"]) <= 2e-4
        R.check(f"fixture {tag} dL/drad", ge, c["ge"], m["ge_terms"], C_RADFAR_E if far else C_RAD_E)


def _near_case(res, nc, seed):
    """Blocks of 256 rays: 512 rays focused inside one pixel at an image corner, a block whose rays all miss, one bundle
    in two clumps 46 pixels apart (the tile holds 48: the far clump's taps fall in and out of it), rays spread over the
    image and its surroundings, a ray count that is no multiple of 256; above 1277 pixels two bundles beyond pixel 1277,
    where the anchor vote's grid clamps.  v.n of either sign and t < 0 come with _near_rays."""
    rng = np.random.default_rng(7000 + seed)
    n, t2, t1 = R.frame(rng)
    p = rng.uniform(-1.0, 1.0, 3)
    span = float(np.float32(rng.uniform(0.5, 4.0)))
    corner = np.array([0.0, res - 1.0]) if seed % 2 else np.array([res - 1.0, res - 1.0])
    blocks = [corner + rng.uniform(-0.45, 0.45, (512, 2))]
    away = np.where(rng.random((256, 1)) < 0.5, -4.5 - rng.uniform(0, 50, (256, 1)), res + 2.5 + rng.uniform(0, 50, (256, 1)))
    blocks.append(np.where(rng.random((256, 2)) < 0.5, away, rng.uniform(-3.0, res + 2.0, (256, 2))))
    blocks[-1][:, 0] = away[:, 0]
    c0 = rng.uniform(0.0, max(res - 50.0, 1.0), 2)
    blocks.append(np.concatenate([c0 + rng.normal(0, 0.5, (128, 2)), c0 + [46.0, 0.0] + rng.normal(0, 2.0, (128, 2))]))
    if res > 1277:
        blocks += [np.array([1500.0, res - 8.0]) + rng.normal(0, 2.0, (256, 2)),
                   np.array([1278.0 + 0.5 * (res - 1278), res - 20.0]) + rng.normal(0, 30.0, (256, 2))]
    blocks.append(rng.uniform(-3.0, res + 2.0, (256 + 77, 2)))
    u = np.concatenate(blocks)
    x, v = R.near_rays(rng, u, p, n, t2, t1, span, res, trange=(-0.25, 0.5))
    rad = rng.normal(size=(len(u), nc)) + 0.5
    rad[rng.random(rad.shape) < 0.05] = 0.0
    if nc >= 3:
        rad[:, 1] = 0.0                                                    # a channel that is all zero
    gI = rng.normal(size=(nc, res, res))
    return dict(x=R.r32(x), v=R.r32(v), rad=R.r32(rad), p=R.r32(p), n=n, t2=t2, t1=t1, res=res, arg=span, gI=R.r32(gI), u=u)


@pytest.mark.gpu
@pytest.mark.parametrize("res,nc", [(1, 1), (2, 2), (7, 5), (48, 3), (49, 32), (64, 3), (300, 2), (2048, 1)])
def test_near_fuzz(gpu, res, nc):
    c = _near_case(res, nc, res + nc)
    assert len(c["x"]) <= 4096
    den = c["v"] @ c["n"]
    assert (den < 0).any() and (den > 0).any() and ((((c["p"] - c["x"]) @ c["n"]) / den) < 0).any()
    outs = _run(gpu, False, c["x"], c["v"], c["rad"], c["p"], c["n"], c["t2"], res, c["arg"], c["gI"])
    m = _model(c["x"], c["v"], c["rad"], c["p"], c["n"], c["t2"], c["t1"], res, c["arg"], False, c["gI"])
    assert m["no_tap"][512:768].all(), "the block whose rays all miss"
    if nc >= 3:
        assert not outs[0][0][1].any() and outs[0][0][0].any(), "a channel that is all zero gives an image of zeros"
    _compare(f"near res {res} C {nc}", outs, m, False)


@pytest.mark.gpu
@pytest.mark.parametrize("res,angle,nc", [(7, 10.0, 2), (48, 120.0, 1), (64, 179.0, 3), (300, 90.0, 5)])
def test_far_fuzz(gpu, res, angle, nc):
    """Angular windows from 10 to 179 degrees, directions inside and outside them, non-unit v of either sign of v.n."""
    rng = np.random.default_rng(8000 + res)
    n, t2, t1 = R.frame(rng)
    p = rng.uniform(-1.0, 1.0, 3)
    m_ = 2048 + 77
    ac = S._ang_cut(angle)
    a = rng.uniform(-1.3, 1.3, (m_, 2)) * ac
    a[: m_ // 10] = rng.uniform(1.5, 3.0, (m_ // 10, 2)) * ac * rng.choice([-1.0, 1.0], (m_ // 10, 2))       # outside
    cn = rng.uniform(0.3, 1.0, m_) * rng.choice([-1.0, 1.0], m_)
    v = np.linalg.solve(np.stack([t1, t2, n]), np.stack([a[:, 0], a[:, 1], cn])).T
    v = R.r32(v * rng.uniform(0.2, 5.0, (m_, 1)))
    x = R.r32(rng.normal(size=(m_, 3)))
    rad = rng.normal(size=(m_, nc)) + 0.5
    if nc >= 3:
        rad[:, 1] = 0.0
    rad, gI, p = R.r32(rad), R.r32(rng.normal(size=(nc, res, res))), R.r32(p)
    outs = _run(gpu, True, x, v, rad, p, n, t2, res, angle, gI)
    m = _model(x, v, rad, p, n, t2, t1, res, angle, True, gI)
    assert not m["no_tap"].all() and (angle > 170 or m["no_tap"].any())       # (a 179 degree window takes every direction)
    _compare(f"far res {res} angle {angle:g} C {nc}", outs, m, True)


def _grads(gpu, fn, x, v, rad, plane, res, arg, T, gI, want):
    """The gradients of the inputs named in `want` (a subset of "xvr"), the others made without grad."""
    xs, vs, rs = (R.to_dev(a, gpu).requires_grad_(k in want) for a, k in ((x, "x"), (v, "v"), (rad, "r")))
    (fn((xs, vs), rs, plane, res, arg, T) * R.to_dev(gI, gpu)).sum().backward()
    return {k: None if t.grad is None else t.grad.clone() for k, t in (("x", xs), ("v", vs), ("r", rs))}


@pytest.mark.gpu
@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
def test_exact_facts(gpu, far):
    """No tolerance: dL/drad[:, c] of a C-channel call is the 1-channel call's with rad[:, c] and gI[c], bit for bit (G_c
    is one sum in a fixed tap order); outputs asked for alone equal the same outputs asked for together; the far field
    leaves x.grad None; rays that miss get exact zeros (also asserted for every fuzz case)."""
    from adjointnonlinearraytracing_amd import sensor
    fn = sensor.splat_radiance_far if far else sensor.splat_radiance
    if far:
        c = R.fixture("far")
        x, v, rad, p, n, t2, res, arg, gI = (c[k] for k in ("x", "v", "rad", "p", "n", "t", "res", "arg", "gI"))
    else:
        c = _near_case(49, 5, 99)
        x, v, rad, p, n, t2, res, arg, gI = (c[k] for k in ("x", "v", "rad", "p", "n", "t2", "res", "arg", "gI"))
    plane, T = (R.to_dev(p[None], gpu), R.to_dev(n[None], gpu)), R.to_dev(t2[None], gpu)
    g = _grads(gpu, fn, x, v, rad, plane, res, arg, T, gI, "xvr")
    assert g["r"].shape == rad.shape and g["r"].any() and g["v"].any()
    assert (g["x"] is None) if far else bool(g["x"].any())
    for k in range(rad.shape[1]):
        one = _grads(gpu, fn, x, v, rad[:, k], plane, res, arg, T, gI[k], "r")        # rad of shape (N,): image (res, res)
        assert one["x"] is None and one["v"] is None
        assert torch.equal(one["r"], g["r"][:, k]), f"channel {k}"
    for want in ("r", "xv", "x", "v", "vr"):
        alone = _grads(gpu, fn, x, v, rad, plane, res, arg, T, gI, want)
        for k in "xvr":
            if k in want and not (far and k == "x"):
                assert torch.equal(alone[k], g[k]), (want, k)
            else:
                assert alone[k] is None, (want, k)


@pytest.mark.gpu
def test_agrees_with_generate_sensor(gpu):
    """C = 1: image, x.grad, v.grad of splat_radiance(rays, rad) and of generate_sensor(rays, rad.detach()) both meet the
    fuzz bounds against the same restatement, and channel c of a C-channel image meets them against the 1-channel
    restatement."""
    from adjointnonlinearraytracing_amd import sensor
    c = _near_case(64, 3, 123)
    x, v, p, n, t2, t1, res, span = (c[k] for k in ("x", "v", "p", "n", "t2", "t1", "res", "arg"))
    rad = c["rad"].copy()
    rad[:, 1] = R.r32(np.random.default_rng(5).normal(size=len(rad)))
    plane, T = (R.to_dev(p[None], gpu), R.to_dev(n[None], gpu)), R.to_dev(t2[None], gpu)
    with torch.no_grad():
        img3 = R.to_np(sensor.splat_radiance((R.to_dev(x, gpu), R.to_dev(v, gpu)), R.to_dev(rad, gpu), plane, res, span, T))
    for k in range(3):
        gI = c["gI"][k:k + 1]
        m = _model(x, v, rad[:, k:k + 1], p, n, t2, t1, res, span, False, gI)
        R.check(f"channel {k} of 3 against the 1-channel restatement", img3[k], m["img"][0], m["img_terms"][0], C_RAD_IMG)
        for name, fn in (("splat_radiance", lambda r, e: sensor.splat_radiance(r, e, plane, res, span, T)),
                         ("generate_sensor", lambda r, e: sensor.generate_sensor(r, e.detach(), plane, res, span, T))):
            xs, vs = R.to_dev(x, gpu).requires_grad_(True), R.to_dev(v, gpu).requires_grad_(True)
            img = fn((xs, vs), R.to_dev(rad[:, k], gpu).requires_grad_(True))
            assert img.shape == (res, res)
            (img * R.to_dev(gI[0], gpu)).sum().backward()
            R.check(f"{name} image", R.to_np(img), m["img"][0], m["img_terms"][0], C_RAD_IMG)
            R.check(f"{name} dL/dx", R.to_np(xs.grad), m["gx"], m["gx_terms"], C_RAD_G, m["keep"])
            R.check(f"{name} dL/dv", R.to_np(vs.grad), m["gv"], m["gv_terms"], C_RAD_G, m["keep"])


@pytest.mark.gpu
def test_call_path(gpu):
    """Under torch.no_grad(); and behind EmissionTracerC on a 9^3 grid: an image loss reaches the emission and the
    absorption coefficient through rad, finite and non-zero."""
    from adjointnonlinearraytracing_amd import sensor, tracer
    R_, side, res = 9, 24, 16
    h = 1.0 / (R_ - 1)
    g = torch.linspace(0.0, 1.0, R_, device=gpu)
    z, y, x_ = torch.meshgrid(g, g, g, indexing="ij")
    r = torch.sqrt((x_ - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) / 0.4
    rif = torch.sqrt(2.0 - torch.clamp(r, max=1.0) ** 2).contiguous()
    e = (0.5 + 0.5 * x_).contiguous().requires_grad_(True)
    a = (0.3 + 0.2 * z).contiguous().requires_grad_(True)
    s = torch.linspace(0.2, 0.8, side, device=gpu)
    px, pz = torch.meshgrid(s, s, indexing="ij")
    pos = torch.stack([px.reshape(-1), torch.full((side * side,), -0.01, device=gpu), pz.reshape(-1)], -1).contiguous()
    vel = torch.zeros_like(pos); vel[:, 1] = 1.0
    xt, vt, rad, tau = tracer.EmissionTracerC.apply(rif, e, a, pos, vel, h, h / 2)
    plane = (torch.tensor([[0.5, 1.2, 0.5]], device=gpu), torch.tensor([[0.0, 1.0, 0.0]], device=gpu))
    T = torch.tensor([[0.0, 0.0, 1.0]], device=gpu)
    with torch.no_grad():
        quiet = sensor.splat_radiance((xt, vt), torch.stack([rad, torch.exp(-tau)], 1), plane, res, 1.0, T)
    assert quiet.shape == (2, res, res) and not quiet.requires_grad and torch.isfinite(quiet).all() and quiet[0].sum() > 0
    img = sensor.splat_radiance((xt, vt), torch.stack([rad, torch.exp(-tau)], 1), plane, res, 1.0, T)
    assert torch.equal(img.detach(), quiet) or torch.allclose(img.detach(), quiet, rtol=1e-5, atol=1e-6)   # atomics: order
    far = sensor.splat_radiance_far((xt, vt), rad, plane, res, 120, T)
    assert far.shape == (res, res)
    ((img ** 2).sum() + (far ** 2).sum()).backward()
    for t in (e, a):
        assert t.grad is not None and torch.isfinite(t.grad).all() and float(t.grad.abs().sum()) > 0
