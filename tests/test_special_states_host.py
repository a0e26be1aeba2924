"""tests/special_states.py on the CPU: the states hold the special values they are made for, and the oracle the GPU tests compare
with is usable on them — finite everywhere, and keeping the signed zeros whose loss the GPU tests are there to catch."""
import numpy as np
import pytest

import special_states as SS
from sweep_reference import STATE, real_mask

CASES = [(axis, nx, ny, g, dtype) for axis in (0, 1) for (nx, ny) in SS.SHAPES[axis] for g in SS.GHOSTS for dtype in SS.DTYPES]
IDS = [f"{'XY'[a]}-{nx}x{ny}-g{g}-{d}" for a, nx, ny, g, d in CASES]


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("axis,nx,ny,g,dtype", CASES, ids=IDS)
def test_the_oracle_is_finite_and_keeps_the_signed_zeros(axis, nx, ny, g, dtype):
    """Every state x triple: finite rho, u, v, E, p, c on the real cells and a finite CFL step. State 1 comes back bit for bit;
    state 2 in rho, E and the transverse velocity, -0 included; state 3 keeps the transverse velocity -0 in every real cell."""
    inside = real_mask(nx, ny, g, axis)
    _ua, ut = SS.along_across(axis)
    for state in SS.STATES:
        for triple in SS.TRIPLES:
            f, ref, dt = SS.special_reference(state, nx, ny, g, axis, triple, dtype)
            what = (SS.STATES[state], triple)
            for k in STATE + ("p", "c"):
                assert np.isfinite(getattr(ref, k)[inside]).all(), (what, k)
            assert np.isfinite(ref.cfl()) and ref.cfl() > 0 and dt > 0, what
            same = {1: STATE, 2: ("rho", "E", ut)}.get(state, ())
            for k in same:
                assert np.array_equal(bits(getattr(ref, k))[inside], bits(f[k])[inside]), (what, k)
            if state == 2:
                assert np.signbit(getattr(ref, ut)[inside]).any() and not np.signbit(getattr(ref, ut)[inside]).all(), what
            if state == 3:
                # -0 in every real cell; the second-order projection may turn it into +0 inside its stencil around the step
                # (it does in the one cell above it: a difference of two equal advection fluxes), nowhere else
                n = (nx, ny)[axis]
                w = 2 if triple[2] == "euler_2nd" else 0
                away = inside & ~(real_mask(nx, ny, g, axis, n // 2 - w, n // 2 + w + 1) if w else np.zeros_like(inside))
                minus_zero = bits(np.array([-0.0], dtype=dtype))[0]
                assert (getattr(ref, ut)[inside] == 0).all(), what
                assert (bits(getattr(ref, ut))[away] == minus_zero).all() and away.sum() >= inside.sum() * (n - 5) // n, what


@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
def test_the_states_hold_their_special_values(axis):
    nx, ny = SS.SHAPES[axis][1]
    g = 5
    n = (nx, ny)[axis]
    ua, ut = SS.along_across(axis)
    row = nx + 2 * g

    def grid(a):
        a = a.reshape(ny + 2 * g, row)[g:g + ny, g:g + nx]
        return a if axis == 0 else a.T                    # [across, along]

    for dtype in SS.DTYPES:
        f = {s: SS.special_state(s, nx, ny, g, axis, dtype) for s in SS.STATES}
        for s in SS.STATES:
            for k in STATE:
                assert f[s][k].dtype == np.dtype(dtype) and f[s][k].size == (nx + 2 * g) * (ny + 2 * g)
            if s != 6:                                     # the same numbers in both precisions
                g64 = SS.special_state(s, nx, ny, g, axis, "float64")
                assert all(np.array_equal(f[s][k].astype(np.float64), g64[k]) for k in STATE)
        assert not np.signbit(f[1][ua]).any() and not np.signbit(f[1][ut]).any()
        for k in (ua, ut):                                 # both zeros, in the last cells along the axis too
            z = grid(f[2][k])
            assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
            assert np.signbit(z[:, -4:]).any() and not np.signbit(z[:, -4:]).all()
        assert np.signbit(grid(f[3][ut])).all() and not np.signbit(grid(f[3][ua])).any() and (grid(f[3][ut]) == 0).all()
        assert set(np.unique(grid(f[3]["rho"]))) == {0.125, 1.0}
        c = grid(f[4][ua])
        assert (c[:, :n // 2] == 0.5).all() and (c[:, n // 2:] == -0.5).all() and set(np.unique(grid(f[4][ut]))) == {-0.25, 0.25}
        r = np.diff(grid(f[5][ua]).astype(np.float64), axis=1)
        assert set(np.unique(r)) == {1 / 128, 1 / 64}      # slope ratios 1, 1/2 and 2 at and next to the middle
        assert (np.diff(grid(f[5]["rho"]).astype(np.float64), axis=1) == 1 / 64).all()
        e = f[5]["E"].astype(np.float64) - 0.5 * (f[5]["u"].astype(np.float64) ** 2 + f[5]["v"].astype(np.float64) ** 2)
        assert (e > 0.5).all()                             # a sound speed exists in every cell, ghosts included
        tiny = float(np.finfo(dtype).smallest_subnormal)
        for k in (ua, ut):
            m = f[6][k].astype(np.float64) / tiny
            assert (m == np.round(m)).all() and np.abs(m).max() <= 2000 and (m < 0).any() and (m > 0).any() and len(np.unique(m)) > 1000
