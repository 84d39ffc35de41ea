"""The host builds of the grid ray-state adjoints against their own past: tests/golden/ray_adjoints_host.npz holds what
backtrace_rays, backtrace_pln_rays, backtrace_sdf_rays, backtrace_target_rays (with and without the seed on dist2) and
backtrace_opl (the term-carrying representative of the integral family) of tests/hostcheck returned when the fixture was
recorded (tests/golden/make_golden.py ray_adjoints_host), and every array must come out byte for byte.  The other referees
compare these routines with float64 autograd within GRAD_TOL and the kernels with the host builds bit for bit; this one is
what a refactor of the reverse march has to keep.  CPU only.

Each case is recorded as its scene builder makes it and once more with dx[::7] = inf, dx[3::11] = nan.  Two things keep the
fixture small, neither loses a bit:
  * the rays of a call do not see each other's seeds, so of the second recording the fixture keeps the rows of the rays
    whose seed was replaced, and the test holds the other rows against the first recording;
  * (dpos, dvel) are stored as their bit pattern XOR that of the seeds (dx, dv), which the builders give: zeros for every
    ray whose gradient is the identity."""
import os

import numpy as np
import pytest

from ray_pin_common import COUNTS, ROUTINES, SCENES, record, replaced, run

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_adjoints_host.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("routine", list(ROUTINES))
@pytest.mark.parametrize("name", SCENES)
def test_host_build_is_the_recorded_one(golden, name, routine):
    got = record(name, routine)
    want = {k: v for k, v in golden.items() if k.startswith(f"{name}.{routine}.")}
    assert sorted(got) == sorted(want) and len(got) == 4
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k
    # the rays whose seed stayed: what the first recording holds
    (b, _), (v, seeds) = run(name, routine, "built"), run(name, routine, "nonfinite")
    keep = ~replaced(len(seeds))
    for f in ("dpos", "dvel") + COUNTS:
        if f in b:
            assert v[f][keep].tobytes() == b[f][keep].tobytes(), f
    assert not np.isfinite(v["dpos"][~keep]).all()


def test_fixture_holds_nothing_else(golden):
    assert {k.split(".")[0] for k in golden} == set(SCENES) and {k.split(".")[1] for k in golden} == set(ROUTINES)
