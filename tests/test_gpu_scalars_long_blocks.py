"""armon_hip_sweep_scalars on blocks that outgrow an extent of its launch grids (csrc/scalar_sweep.hpp, scalar_launch), against
the restatement (tests/scalars_restated.py). No other block the scalar sweep meets in the suite has more than 101 rows or 530
columns; the code has paths that begin far beyond:

 * k_scalar_x carries 4 rows per workgroup in grid.y, capped at 32768 groups, and the rest in grid.z; the kernel rebuilds
   ``row = (blockIdx.z * gridDim.y + blockIdx.y) * 4 + threadIdx.y`` and returns past ny;
 * k_scalar_y splits a tall block into about a thousand runs of a few hundred rows (scalar_y_seg), each with its own
   buffer descriptors, and a wide one into a thousand workgroups of one run of ``seg = ny`` rows;
 * the X sweep of a wide block has 2501 strips per row, with 16-B loads and stores on the interior ones if the pitch is even.

The shapes (nx, ny, nghost) are the smallest that cross each threshold:

 ==== ================ ==========================================================================================
 Z2   (10, 131077, 4)  32770 row groups: grid.z = 2, two groups in the last layer, cut at ny mid-workgroup
 F2   (10, 262144, 4)  65536 row groups: grid.z = 2 and the last layer full to its last group, the last block whose
                       ``(groups + gy - 1) / gy`` is 2 (a layer stride one group short still covers Z2 and T2, whose
                       last layers have room to spare: it loses the last group of this one)
 T2   (10, 262147, 4)  grid.z = 3, a full middle layer; Y runs of 257 rows on 1021 workgroups (on 256 CUs)
 W1   (300007, 6, 5)   odd pitch, no ``vec``; 2501 strips per row; Y grid.x = 1172; seg = ny = 6
 W2   (300008, 6, 4)   even pitch: ``vec`` loads and stores on all interior strips
 ==== ================ ==========================================================================================

Every output plane starts as the harness' marker and is compared as integers. The references hold up to 38 MB per array:
the cached ones are dropped whenever the shape changes (``blocks``). Tuned arithmetic prints what it measures (pytest -s)."""
import functools

import numpy as np
import pytest

from scalars_harness import (WALLS, Planes, assert_untouched, case_numbers, descriptor, exact_launch_is_the_restatement, launch,
                             plane_kappa, rand_planes)
from scalars_restated import restated_sweep
from sweep_harness import F_HIGH, F_LOW, MARKER, Block, bits
from sweep_reference import rand_state, real_mask
from test_gpu_scalars import problem_of, run, same_bits, smooth_state

pytestmark = pytest.mark.gpu

SHAPES = dict(Z2=(10, 131077, 4), F2=(10, 262144, 4), T2=(10, 262147, 4), W1=(300007, 6, 5), W2=(300008, 6, 4))
SEEDS = dict(Z2=9300, T2=9310, W1=9320, W2=9330, F2=9340)
DTYPES = ("float64", "float32")
GAD = ("GAD", "minmod", "euler_2nd", "perfect_gas")
GODUNOV = ("Godunov", "minmod", "euler", "bizarrium")

assert [(-(-ny // 4) - 1) // 32768 + 1 for _nx, ny, _g in SHAPES.values()] == [2, 2, 3, 1, 1]       # grid.z of the X sweep
assert -(-SHAPES["Z2"][1] // 4) - 32768 == 2 and SHAPES["Z2"][1] % 4 == 1                            # two groups, the last of one row
assert SHAPES["F2"][1] == 2 * 32768 * 4                                                              # two full layers
assert [-(-(nx + g % 8) // 120) for nx, _ny, g in (SHAPES["W1"], SHAPES["W2"])] == [2501, 2501]
assert -(-(SHAPES["W1"][0] + SHAPES["W1"][2] % 16) // 256) == 1172


@functools.lru_cache(maxsize=None)
def inputs_of(name, eos, dtype, ns):
    """(state, planes) of a shape: random over the whole ghosted block, shared and never modified."""
    nx, ny, g = SHAPES[name]
    f = rand_state(nx, ny, g, eos, dtype, SEEDS[name])
    planes = rand_planes(nx, ny, g, ns, dtype, SEEDS[name] + 1)
    for a in list(f.values()) + planes:
        a.setflags(write=False)
    return f, planes


@functools.lru_cache(maxsize=None)
def kappa_of(name, axis):
    """plane_kappa of the two random planes of the tuned test: from the two restatements alone."""
    nx, ny, g = SHAPES[name]
    f32, planes32 = inputs_of(name, GAD[3], "float32", 2)
    dt, dx = case_numbers(nx, ny, axis, GAD[3], "float32")
    kappa, _ = plane_kappa(f32, planes32, nx, ny, g, axis, *GAD, dt, dx, **WALLS)
    assert all(k > 0.5 for k in kappa), kappa              # a yardstick, not an accident of one cell
    return kappa


def drop_references():
    inputs_of.cache_clear()
    kappa_of.cache_clear()


@pytest.fixture(scope="module")
def dev():
    import armon_amd
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.wait()
    d.close()


@pytest.fixture(scope="module")
def blocks(dev):
    """``blocks(name, dtype)``: the Block of a shape. Entering another shape drops the references and the blocks of the last."""
    cache, last = {}, [None]

    def get(name, dtype):
        if last[0] != name:
            dev.wait()
            cache.clear()
            drop_references()
            last[0] = name
        key = np.dtype(dtype).name
        if key not in cache:
            cache[key] = Block(dev, *SHAPES[name], dtype)
        return cache[key]

    yield get
    dev.wait()
    cache.clear()
    drop_references()


def case_id(v):
    if isinstance(v, tuple):
        return v[0]
    return "XY"[v] if isinstance(v, int) and v < 2 else (f"ns{v}" if isinstance(v, int) else str(v))


EXACT_CASES = [(name, dtype, axis, opts, ns) for name in SHAPES for opts, ns in ((GAD, 1), (GODUNOV, 4))
               if ns == 1 or name in ("Z2", "W1") for dtype in DTYPES for axis in (0, 1)]


@pytest.mark.parametrize("name,dtype,axis,opts,ns", EXACT_CASES, ids=case_id)
def test_exact_scalar_sweep_of_a_long_block_is_the_restatement(blocks, name, dtype, axis, opts, ns):
    """phi_out of one exact launch: the restatement's bits on every real cell, the marker everywhere else; phi_in, the eight
    state arrays, p, c and the dt scalar untouched. Both sides mirrored. Z2 and W1 also carry four planes through Godunov,
    first-order remap and Bizarrium (each the ns = 1 launch on it)."""
    nx, ny, g = SHAPES[name]
    blk = blocks(name, dtype)
    f, planes = inputs_of(name, opts[3], dtype, ns)
    dt, dx = case_numbers(nx, ny, axis, opts[3], dtype)
    want, _ = restated_sweep(f, planes, nx, ny, g, axis, *opts, dt, dx, 1, 1, F_LOW, F_HIGH, dtype)
    exact_launch_is_the_restatement(blk, f, planes, want, axis, *opts, dt, what=f"{name} {dtype} {'XY'[axis]}: ")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("name", ["Z2", "W2"])
def test_tuned_scalar_sweep_of_a_long_block(blocks, name, axis, dtype):
    """As test_tuned_scalar_sweep (tests/test_gpu_scalars.py): under walls whose transverse factor is +1 the plane that holds
    the transverse velocity is armon_hip_sweep's transverse velocity, bit for bit; two random planes stay within 4 kappa eps of
    the field maximum from the fp64 restatement of the input the kernel got, kappa from the two restatements alone."""
    nx, ny, g = SHAPES[name]
    blk = blocks(name, dtype)
    opts = (axis,) + GAD
    f, planes = inputs_of(name, GAD[3], dtype, 2)
    dt, dx = case_numbers(nx, ny, axis, GAD[3], dtype)
    t_name = "v" if axis == 0 else "u"
    inside = real_mask(nx, ny, g, axis)
    mark = MARKER[blk.dtype.name]
    P = Planes(blk, 3)
    try:
        blk.upload(f)
        blk.mark_outputs()
        P.upload([f[t_name]] + planes)
        d = descriptor(blk, *opts, False, dt, **WALLS)
        launch(blk, d, P.inp, P.out)
        _, got = P.fetch()
        assert_untouched(blk, f, "tuned scalar sweep")
        blk.sweep(*opts, False, dt, **WALLS)               # the state sweep of the same descriptor
        state = blk.fetch()
        assert np.array_equal(bits(got[0])[inside], bits(state[t_name])[inside]), "the plane of ut is not the sweep's ut"
        for k in range(3):
            assert ((bits(got[k]) == mark) == ~inside).all(), f"phi_out[{k}]: not exactly the real cells were written"
    finally:
        P.free()
    kappa = kappa_of(name, axis)
    ref, _ = restated_sweep({k: a.astype(np.float64) for k, a in f.items()}, [p.astype(np.float64) for p in planes], nx, ny, g, *opts,
                            dt, dx, 1, 1, WALLS["f_low"], WALLS["f_high"], "float64")
    eps = float(np.finfo(blk.dtype).eps)
    for k in range(2):
        want = ref[k][inside]
        r = float(np.abs(got[k + 1][inside].astype(np.float64) - want).max() / (eps * np.abs(want).max()))
        print(f"\n{name} {dtype} {'XY'[axis]}: plane {k} {r:.2f} eps of the field maximum (kappa {kappa[k]:.2f}: {r / kappa[k]:.2f} "
              f"of it, bound 4 kappa)")
        assert r <= 4 * kappa[k], (k, r, kappa[k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("splitting", ["X_only", "Y_only"])
def test_a_plane_that_starts_as_the_transverse_velocity_stays_it_on_a_long_block(splitting, exact, dtype):
    """Three cycles of the solver on Z2's cells: the scalar sweep of a block whose rows overflow into grid.z, fed by the solver's
    own descriptors; the plane is the velocity bit for bit, and it has moved."""
    N = SHAPES["Z2"][:2]
    s = smooth_state(N, dtype)
    t_name = "v" if splitting == "X_only" else "u"
    stats, out = run(test=problem_of(s, {"phi": s[t_name]}), N=N, data_type=dtype, axis_splitting=splitting, exact_arithmetic=exact,
                     maxcycle=3, cfl=0.4)
    assert stats.cycles == 3 and stats.scalars == ("phi",)
    assert not same_bits(out[t_name], s[t_name].astype(dtype))          # it moved
    assert same_bits(out["s:phi"], out[t_name])
