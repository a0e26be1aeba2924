"""Every kernel on blocks that outgrow the y extent of a launch grid, against the CPU oracle, bit for bit.

No other block of the suite has more than 16384 rows or columns; the code has paths that begin beyond that:

 * ``range_grid`` (csrc/common.hpp) caps ``grid.y`` at 65535 and every staged kernel strides over the remaining rows;
 * the fused fp32 X sweep gives up its workgroup of four strips of one row when ``ny > 65535``;
 * the fused X sweep (main form ``ceil(ny / 4)``, narrow form ``ceil(ny / 16)`` rows of workgroups) and the staged Y marches
   (``ceil(col_len / 8)``) launch a ``grid.y`` that is not capped;
 * ``k_dtCFL_partial`` takes more than 4 rows per workgroup on a tall block with a geometry of its own;
 * ``linear_grid`` is capped at ``8 n_cu`` workgroups: on a face of 262147 cells every thread loops;
 * the Y march does the arithmetic inside a run in 32 bits: rows of 300017 cells.

The shapes (nx, ny, nghost) are the smallest that cross each threshold:

 ==== ================ ==========================================================================================
 T1   (10, 65541, 5)   col_len > 65535 in every range_grid launch; the fp32 X fallback; the main X form; odd ghost width
 T2   (10, 262147, 4)  the main X sweep's grid.y = 65537; dtCFL with 9 rows per workgroup; fp32 two columns per lane in Y
 T3   (4, 1048583, 4)  fp32 only: the narrow X form's grid.y = 65537
 T4   (4, 524301, 4)   the staged Y marches' grid.y > 65535 for the flux range
 W1   (300007, 6, 5)   odd pitch: strip origins row by row, store exchange; 2501 X strips per row; a Y grid.x of 1172
 W2   (300008, 6, 4)   the same with an even pitch that is not a multiple of a sector; fp32 pairs
 ==== ================ ==========================================================================================

The machinery is that of tests/test_gpu_sweep_random_state.py (``Block``, ``reference``, ``check_outputs``, ``run_tuned_forms``,
``kappa_of``, ``assert_within_rounding``, ``plant_cell``; outputs start as a NaN with a payload and are compared as
integers). The references hold 20-50 MB per array: the cached ones are dropped whenever the shape changes (``blocks``).
"""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_sweep_random_state as R
from sweep_reference import STATE, SweepResult, draw_state, reference_sweep
from test_gpu_sweep_random_state import (F_HIGH, F_LOW, OUT_NAMES, Block, assert_within_rounding, bits, check_outputs, kappa_of,
                                         lag_of, plant_cell, reference, run_tuned_forms)

pytestmark = pytest.mark.gpu

SHAPES = dict(T1=(10, 65541, 5), T2=(10, 262147, 4), T3=(4, 1048583, 4), T4=(4, 524301, 4), W1=(300007, 6, 5), W2=(300008, 6, 4))
SEEDS = {name: 9100 + k for k, name in enumerate(SHAPES)}
DTYPES = ("float64", "float32")
GAD = ("GAD", "minmod", "euler_2nd", "perfect_gas")
GODUNOV = ("Godunov", "minmod", "euler", "bizarrium")


def drop_references():
    for cached in (R.state_of, R.reference, R.kappa_of):
        cached.cache_clear()


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


def ref_of(name, axis, opts, dtype, ref_dtype=None):
    """``reference`` of a shape, both sides mirrored, spelled as ``kappa_of`` spells its calls so that the cache serves both."""
    nx, ny, g = SHAPES[name]
    return reference(nx, ny, g, axis, *opts, dtype, SEEDS[name], bc=(1, 1), ref_dtype=ref_dtype or dtype)


def case_id(v):
    if isinstance(v, tuple) and v and isinstance(v[0], str):
        return v[0] + "-" + v[3]
    return "XY"[v] if isinstance(v, int) else str(v)


# ---- 1. fused sweep, exact arithmetic ------------------------------------------------------------------------------------

EXACT_CASES = ([("T1", dt, ax, opts) for opts in (GAD, GODUNOV) for dt in DTYPES for ax in (0, 1)] +
               [("T2", dt, ax, GAD) for dt in DTYPES for ax in (0, 1)] +
               [("T3", "float32", 0, GAD)] +
               [("W1", dt, ax, opts) for opts in (GAD, GODUNOV) for dt in DTYPES for ax in (0, 1)] +
               [("W2", "float32", ax, GAD) for ax in (0, 1)])


@pytest.mark.parametrize("name,dtype,axis,opts", EXACT_CASES, ids=case_id)
def test_exact_sweep_of_a_long_block_is_the_oracles(blocks, name, dtype, axis, opts):
    """rho, u, v, E, p_out, c_out and dt_cfl_out of one exact sweep: the oracle's bits on every real cell, the marker
    everywhere else. T1 and T2 in fp32 along X take one strip of four rows per workgroup (the fallback of blocks with more
    than 65535 rows); T2 along X launches 65537 rows of workgroups, T3 (the narrow form: the block is 4 cells wide) too."""
    blk = blocks(name, dtype)
    f, ref, dt = ref_of(name, axis, opts, dtype)
    blk.upload(f)
    blk.mark_outputs()
    blk.sweep(axis, *opts, True, dt, emit=(1, 1))
    check_outputs(blk, blk.fetch(), ref, axis, emit=(1, 1))


# ---- 2. fused sweep, tuned arithmetic ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("name", ["T1", "T2", "W1", "W2"])
def test_tuned_forms_agree_on_a_long_block_and_stay_within_the_rounding_of_the_operation(blocks, name, axis, dtype):
    """Tuned arithmetic in every launch form of TUNED_FORMS: the same bits in all of them, and the fp64 reference on the input
    the kernel got within the per-sweep bound of assert_within_rounding, whose yardstick (kappa_of) comes from the two oracles
    alone. On T1 and T2 in fp32 along X, ARMON_X_ROWS=2 (four strips of one row) is silently the fallback, one strip of four
    rows: a block with more than 65535 rows cannot carry its rows in grid.y, so there two of the three forms are one launch.
    W1 and W2 take the store exchange in Y by themselves (their pitch is no multiple of a sector); W2 and T2 the fp32 march with
    two columns per lane."""
    nx, ny, g = SHAPES[name]
    blk = blocks(name, dtype)
    opts = (axis,) + GAD
    f, ref64, dt = ref_of(name, axis, GAD, dtype, "float64")
    blk.upload(f)
    out = run_tuned_forms(blk, opts, dt, (1, 1), "")
    assert_within_rounding(blk, out, ref64, kappa_of(nx, ny, g, *opts, SEEDS[name]), axis, f"tuned {dtype} {'XY'[axis]} {name}")


# ---- 3. partial sweeps ---------------------------------------------------------------------------------------------------

PIECES = {("T2", 1): [(65530, 65545), (262139, 262147), (262146, 262147)],      # across row 65535; the last 8 rows; the last row
          ("T1", 0): [(0, 4), (6, 10)]}                                          # the narrow form on a tall block


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,axis", list(PIECES), ids=["T2-Y", "T1-X"])
def test_a_partial_sweep_of_a_long_block_writes_its_piece_and_nothing_else(blocks, name, axis, dtype, exact):
    """Every piece leaves the marker in every cell outside (real cells x [out_lo, out_hi) along the axis) and in no cell inside;
    in exact arithmetic the cells inside hold the full sweep's bits and dt_cfl_out the minimum over the piece."""
    blk = blocks(name, dtype)
    f, ref, dt = ref_of(name, axis, GAD, dtype)
    blk.upload(f)
    for lo, hi in PIECES[name, axis]:
        blk.mark_outputs()
        blk.sweep(axis, *GAD, exact, dt, emit=(1, 1), out_range=(lo, hi))
        check_outputs(blk, blk.fetch(), ref, axis, lo, hi, emit=(1, 1), exact=exact, what=f"piece [{lo}, {hi}): ")


# ---- 4. the CFL reduction finds one planted cell ----------------------------------------------------------------------------

ROWS = {"T1": (0, 65534, 65535, 65536, 65540), "T2": (0, 65534, 65535, 65536, 262146, 262140, 262143),
        "T4": (0, 65534, 65535, 65536, 524300)}
COLUMNS = {"W1": (0, 119, 120, 299999, 300006)}


def positions(name):
    """(x, y) of the planted cells: the rows of a tall shape (the column moves with the row), the columns of a wide one."""
    nx, ny, _g = SHAPES[name]
    if name in ROWS:
        return [(r % nx, r) for r in ROWS[name]]
    return [(c, c % ny) for c in COLUMNS[name]]


assert all(p[1] == SHAPES[n][1] - 1 for n in ROWS for p in positions(n)[4:5])
assert positions("W1")[4][0] == SHAPES["W1"][0] - 1


def planted_reference(name, axis, dtype, pos):
    """(input, reference, dt) of the state of ``ref_of`` with plant_cell at ``pos``, the CFL reduction with the cell size along
    the axis both ways. A sweep couples the cells of one line along its axis only, so the reference of the planted state is
    the reference of the state itself with that one line replaced by the oracle's sweep of the line taken as a block of its
    own: a block one cell across, with the same ghost cells along the axis. That the oracle gives a line the same bits either
    way is asserted: away from the planted cell (more than 2 LAG cells) the line's sweep must equal the whole block's."""
    nx, ny, g = SHAPES[name]
    f0, base, dt = ref_of(name, axis, GAD, dtype)
    f = plant_cell(f0, nx, ny, g, axis, "perfect_gas", pos)
    T = np.dtype(dtype).type
    size = float(T(1.) / T((nx, ny)[axis]))
    rows, pitch = ny + 2 * g, nx + 2 * g
    x, y = pos
    if axis == 0:
        line_in = {k: f[k].reshape(rows, pitch)[y:y + 2 * g + 1].copy().ravel() for k in STATE}
        lnx, lny = nx, 1
    else:
        line_in = {k: np.ascontiguousarray(f[k].reshape(rows, pitch)[:, x:x + 2 * g + 1]).ravel() for k in STATE}
        lnx, lny = 1, ny
    line = reference_sweep(line_in, lnx, lny, g, axis, *GAD, dt, size, 1, 1, F_LOW, F_HIGH, np.dtype(dtype))
    a, n, lag = pos[axis], (nx, ny)[axis], lag_of("GAD", "euler_2nd")
    far = np.abs(np.arange(n) - a) > 2 * lag
    arrays = {}
    for k in OUT_NAMES:
        whole = getattr(base, k).copy().reshape(rows, pitch)
        part = getattr(line, k).reshape(lny + 2 * g, lnx + 2 * g)
        new = part[g, g:g + nx] if axis == 0 else part[g:g + ny, g]
        old = whole[g + y, g:g + nx] if axis == 0 else whole[g:g + ny, g + x]
        assert np.isfinite(new).all(), k
        assert np.array_equal(bits(new[far]), bits(old[far])), f"{k}: the oracle's sweep of one line is not its sweep of the block"
        old[:] = new
        arrays[k] = whole.ravel()
    ut = "v" if axis == 0 else "u"
    assert arrays[ut].reshape(rows, pitch)[g + y, g + x] != getattr(base, ut).reshape(rows, pitch)[g + y, g + x]
    ref = SweepResult(nx=nx, ny=ny, g=g, axis=axis, dtype=np.dtype(dtype), f32=np.dtype(dtype) == np.float32, cfl_dx=size,
                      cfl_dy=size, **arrays)
    return f, ref, dt


def end_pieces(n, lag):
    """A LAG-wide piece at either end and the interior between them, the interior first; a block with fewer than 2 LAG + 1
    cells along the axis (W1 along Y: 6 rows) has no interior, and its high piece begins where the low one ends."""
    low, high = (0, min(lag, n)), (max(n - lag, lag), n)
    return ([(lag, n - lag)] if n - lag > lag else []) + [low] + ([high] if high[0] < high[1] else [])


PLANT_CASES = [(name, axis, k) for name in ("T1", "T2", "W1") for axis in (0, 1) for k in range(len(positions(name)))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,axis,where", PLANT_CASES, ids=[f"{n}-{'XY'[a]}-{'row' if n in ROWS else 'column'}{positions(n)[k][n in ROWS]}"
                                                              for n, a, k in PLANT_CASES])
def test_cfl_reduction_of_a_long_block_finds_the_one_decisive_cell(blocks, name, axis, where, dtype):
    """One cell carries the minimum (asserted on the reference), in row 0, 65534, 65535, 65536, ny - 1 of T1 and T2 (T2 also
    262140 and 262143: the last rows of workgroups of the X sweep), in column 0, 119, 120, 299999, nx - 1 of W1. dt_cfl_out of
    the full sweep is the reference's, and so is the minimum accumulated over the pieces of end_pieces. A NaN in E of that
    cell leaves a NaN in dt_cfl_out, of the full sweep and of the pieces."""
    nx, ny, g = SHAPES[name]
    pos = positions(name)[where]
    blk = blocks(name, dtype)
    f, ref, dt = planted_reference(name, axis, dtype, pos)
    n, lag, a = (nx, ny)[axis], lag_of("GAD", "euler_2nd"), pos[axis]
    assert ref.cfl(a, a + 1) == ref.cfl() and (a == 0 or ref.cfl(0, a) > ref.cfl()) and (a == n - 1 or ref.cfl(a + 1, n) > ref.cfl())
    cfl = (blk.cell_size(axis),) * 2                       # the same size both ways: the fastest cell decides, along or across
    assert cfl[0] == ref.cfl_dx
    pieces = end_pieces(n, lag)
    assert pieces[-1][1] == n and sorted(pieces)[0][0] == 0 and sum(hi - lo for lo, hi in pieces) == n
    blk.upload(f)
    blk.mark_outputs()
    blk.sweep(axis, *GAD, True, dt, cfl_sizes=cfl)
    check_outputs(blk, blk.fetch(), ref, axis, what="full sweep: ")
    blk.mark_outputs()
    for k, piece in enumerate(pieces):
        blk.sweep(axis, *GAD, True, dt, out_range=piece, accumulate=k > 0, cfl_sizes=cfl)
    check_outputs(blk, blk.fetch(), ref, axis, what="pieces: ")
    poisoned = f["E"].copy()
    poisoned[(pos[1] + g) * (nx + 2 * g) + pos[0] + g] = np.nan
    blk.grid.data["E"].copy_from_host(poisoned)
    blk.mark_outputs()
    blk.sweep(axis, *GAD, True, dt, cfl_sizes=cfl)
    assert np.isnan(blk.fetch()["dt"][0]), "full sweep: a NaN in E did not reach dt_cfl_out"
    blk.mark_outputs()
    for k, piece in enumerate(pieces):
        blk.sweep(axis, *GAD, True, dt, out_range=piece, accumulate=k > 0, cfl_sizes=cfl)
    assert np.isnan(blk.fetch()["dt"][0]), "pieces: a NaN in E did not reach dt_cfl_out"


# ---- 5. staged kernels through the C ABI ----------------------------------------------------------------------------------

ADV = ("us", "rho", "u", "v", "E", "work_1", "work_2", "work_3", "work_4")
ALL = ("rho", "u", "v", "E", "p", "c", "g", "us", "ps", "work_1", "work_2", "work_3", "work_4")
# entry point, range of ranges_for, arguments: a field, "ua" (the velocity along the axis), a scalar of ``scalars``, or a tag
KERNELS = {"perfect_gas_EOS": ("real", ("gamma", "rho", "E", "u", "v", "p", "c", "g")),
           "bizarrium_EOS": ("real", ("rho", "u", "v", "E", "p", "c", "g")),
           "acoustic": ("fluxes", ("s", "us", "ps", "rho", "ua", "p", "c")),
           "acoustic_GAD-no_limiter": ("fluxes", ("s", "dt", "dx", "us", "ps", "rho", "ua", "p", "c", 0)),
           "acoustic_GAD-minmod": ("fluxes", ("s", "dt", "dx", "us", "ps", "rho", "ua", "p", "c", 1)),
           "acoustic_GAD-superbee": ("fluxes", ("s", "dt", "dx", "us", "ps", "rho", "ua", "p", "c", 2)),
           "cell_update": ("cell_update", ("s", "dx", "dt", "us", "ps", "rho", "ua", "E")),
           "advection_first_order": ("advection", ("s", "dt") + ADV),
           "advection_second_order": ("advection", ("s", "dx", "dt") + ADV),
           "euler_projection": ("real", ("s", "dx", "dt") + ADV)}


def staged_state(nx, ny, g, dtype, seed, eos="perfect_gas", names=ALL):
    """Physically plausible random fields over the whole ghosted block: rand_state of tests/test_gpu_kernels.py with a ghost
    width and a precision."""
    rng = np.random.default_rng(seed)
    n = (nx + 2 * g) * (ny + 2 * g)
    f = {**draw_state(rng, n, eos), "p": rng.uniform(0.1, 2.0, n), "c": rng.uniform(0.5, 2.0, n), "g": rng.uniform(1, 2, n),
         "us": rng.uniform(-1, 1, n), "ps": rng.uniform(0.1, 2.0, n), "work_1": rng.uniform(-1, 1, n),
         "work_2": rng.uniform(-1, 1, n), "work_3": rng.uniform(-1, 1, n), "work_4": rng.uniform(-1, 1, n)}
    return {k: f[k].astype(dtype) for k in names}


def ranges_for(oracle, nx, ny, g, axis, w=2):
    dr = oracle.domain_range
    if axis == 0:
        return dict(s=1, fluxes=dr(nx, ny, g, (-w, 0), (w + 1, 0)), cell_update=dr(nx, ny, g, (-w, 0), (w, 0)),
                    advection=dr(nx, ny, g, (0, 0), (1, 0)), real=dr(nx, ny, g))
    return dict(s=nx + 2 * g, fluxes=dr(nx, ny, g, (0, -w), (0, w + 1)), cell_update=dr(nx, ny, g, (0, -w), (0, w)),
                advection=dr(nx, ny, g, (0, 0), (0, 1)), real=dr(nx, ny, g))


def conv(r):
    from armon_amd._lib import Range
    return Range(r.col_start, r.col_step, r.col_len, r.row_start, r.row_len)


def entry(L, name, dtype):
    return getattr(L, "armon_hip_" + name + ("_f32" if np.dtype(dtype) == np.float32 else ""))


def assert_whole_arrays(d, f, what):
    """Every array of the state, whole: what a kernel wrote outside its range shows up as well."""
    for k in f:
        got = d[k].to_host()
        bad = np.flatnonzero(bits(got) != bits(f[k]))
        assert bad.size == 0, f"{what}: {k} differs from the oracle's in {bad.size} cells, first at flat index {bad[0]}"


def run_staged_kernel(dev, oracle, kernel, shape, axis, dtype, names=ALL):
    import armon_amd
    nx, ny, g = shape
    which, tokens = KERNELS[kernel]
    eos = "bizarrium" if kernel == "bizarrium_EOS" else "perfect_gas"
    f = staged_state(nx, ny, g, dtype, 30 + len(kernel) + axis, eos, names)
    d = {k: dev.from_host(a) for k, a in f.items()}
    ranges = ranges_for(oracle, nx, ny, g, axis)
    scalars = dict(s=ranges["s"], dt=1e-3, dx=0.1, gamma=1.4)              # (a step of CFL number 0.03 whatever the shape)
    fields = [("u", "v")[axis] if t == "ua" else t for t in tokens]
    host = [oracle.ptr(f[t]) if t in f else scalars.get(t, t) for t in fields]
    device = [C.c_void_p(d[t].ptr) if t in d else scalars.get(t, t) for t in fields]
    name = kernel.split("-")[0]
    getattr(oracle.lib(f32=np.dtype(dtype) == np.float32), "armon_oracle_" + name)(ranges[which], *host)
    L = armon_amd.lib()
    assert entry(L, name, dtype)(dev.ctx, conv(ranges[which]), *device) == 0, L.armon_hip_last_error()
    dev.wait()
    assert_whole_arrays(d, f, f"{kernel} along {'xy'[axis]}")


STAGED_T1 = [(k, 0) for k in ("perfect_gas_EOS", "bizarrium_EOS")] + [(k, ax) for k in list(KERNELS)[2:] for ax in (0, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,axis", STAGED_T1, ids=lambda v: "xy"[v] if isinstance(v, int) else v)
def test_staged_kernel_on_more_rows_than_a_grid_has(dev, oracle, kernel, axis, dtype):
    """T1: every range of every kernel has more than 65535 rows, so every workgroup of a range_grid launch takes a second row
    (ARMON_FOR_RANGE, the row loops of the x forms of acoustic_GAD and advection_second_order), and the y forms of those two
    march 8194 runs of 8 rows. The two EOS take no axis. Whole arrays against the oracle's."""
    run_staged_kernel(dev, oracle, kernel, SHAPES["T1"], axis, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,names", [("acoustic_GAD-minmod", ("rho", "v", "p", "c", "us", "ps")), ("advection_second_order", ADV)],
                         ids=["acoustic_GAD", "advection_second_order"])
def test_staged_y_march_with_more_runs_than_65535(dev, oracle, kernel, names, dtype):
    """T4 along y: the marches of acoustic_GAD (flux range: ny + 5 rows) and advection_second_order (ny + 1 rows) launch one
    row of workgroups per run of 8 rows, more than 65535 of them."""
    nx, ny, g = SHAPES["T4"]
    assert (ny + 1 + 7) // 8 > 65535
    run_staged_kernel(dev, oracle, kernel, SHAPES["T4"], 1, dtype, names)


BCV = ("rho", "u", "v", "p", "c", "g", "E")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", [1, 2, 3, 4])
def test_boundary_conditions_of_a_long_block(dev, oracle, side, dtype):
    """T1: the Left and Right borders have 65541 cells, more than the 8 n_cu workgroups of linear_grid hold threads."""
    import armon_amd
    from armon_amd.blocking import BlockSize, Side, axis_of
    nx, ny, g = SHAPES["T1"]
    bs = BlockSize((nx + 2 * g, ny + 2 * g), g)
    sd = Side(side)
    f = staged_state(nx, ny, g, dtype, 8, names=BCV)
    d = {k: dev.from_host(a) for k, a in f.items()}
    r = bs.border_domain(sd).to_c()
    incr = bs.stride_along(axis_of(sd)) * (-1 if sd in (Side.Left, Side.Bottom) else 1)
    uf, vf = (-1., 1.) if sd in (Side.Left, Side.Right) else (1., -1.)
    orr = oracle.Range(r.col_start, r.col_step, r.col_len, r.row_start, r.row_len)
    oracle.lib(f32=np.dtype(dtype) == np.float32).armon_oracle_boundary_conditions(orr, incr, g, uf, vf, *(oracle.ptr(f[k]) for k in BCV))
    L = armon_amd.lib()
    assert entry(L, "boundary_conditions", dtype)(dev.ctx, r, incr, g, uf, vf, *(C.c_void_p(d[k].ptr) for k in BCV)) == 0
    dev.wait()
    assert_whole_arrays(d, f, f"boundary_conditions {sd.name}")


def pack_and_unpack(dev, oracle, shape, side, f, dtype):
    """pack_to_array of the border of ``side`` and unpack_from_array of that buffer into its ghost cells, oracle and device:
    the same buffer, the same arrays. Returns the packed buffer."""
    import armon_amd
    from armon_amd.blocking import BlockSize, Side
    nx, ny, g = shape
    bs = BlockSize((nx + 2 * g, ny + 2 * g), g)
    sd = Side(side)
    names = tuple(f)
    d = {k: dev.from_host(a) for k, a in f.items()}
    face = bs.real_face_size(sd)
    send = bs.border_domain(sd, single_strip=False).to_c()
    recv = bs.ghost_domain(sd, single_strip=False).to_c()
    buf_h = np.zeros(face * g * 7, dtype=dtype)
    buf_d = dev.zeros(face * g * 7, dtype)
    vars_h = (C.c_void_p * 7)(*(f[k].ctypes.data for k in names))
    vars_d = (C.c_void_p * 7)(*(d[k].ptr for k in names))
    osend = oracle.Range(send.col_start, send.col_step, send.col_len, send.row_start, send.row_len)
    orecv = oracle.Range(recv.col_start, recv.col_step, recv.col_len, recv.row_start, recv.row_len)
    OL, L = oracle.lib(f32=np.dtype(dtype) == np.float32), armon_amd.lib()
    OL.armon_oracle_pack_to_array(osend, g, face, oracle.ptr(buf_h), 7, vars_h)
    assert entry(L, "pack_to_array", dtype)(dev.ctx, send, g, face, C.c_void_p(buf_d.ptr), 7, vars_d) == 0
    dev.wait()
    packed = buf_d.to_host()
    assert np.array_equal(bits(packed), bits(buf_h)), f"pack_to_array {sd.name}"
    OL.armon_oracle_unpack_from_array(orecv, g, face, oracle.ptr(buf_h), 7, vars_h)
    assert entry(L, "unpack_from_array", dtype)(dev.ctx, recv, g, face, C.c_void_p(buf_d.ptr), 7, vars_d) == 0
    dev.wait()
    assert_whole_arrays(d, f, f"unpack_from_array {sd.name}")
    return packed


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,side", [("T1", 1), ("T1", 2), ("T1", 3), ("T1", 4), ("T2", 1), ("T2", 2)],
                         ids=lambda v: v if isinstance(v, str) else ("Left", "Right", "Bottom", "Top")[v - 1])
def test_pack_and_unpack_of_a_long_face(dev, oracle, name, side, dtype):
    """The Left and Right faces of T1 (65541 cells) and T2 (262147 cells: each thread of the capped linear grid loops) and the
    short ones of T1, on a random state against the oracle's buffer and arrays. In fp64 also on arrays that hold
    1e8 * variable + cell index (exact below 2^53; the 1e6 of tests/test_gpu_kernels.py would collide with 4.7 million cells):
    the packed buffer is a bijection, nothing is packed twice."""
    nx, ny, g = shape = SHAPES[name]
    pack_and_unpack(dev, oracle, shape, side, staged_state(nx, ny, g, dtype, 11, names=BCV), dtype)
    if dtype == "float64":
        n = (nx + 2 * g) * (ny + 2 * g)
        assert n < 1e8
        f = {k: np.arange(n, dtype=np.float64) + 1e8 * vi for vi, k in enumerate(BCV)}
        packed = pack_and_unpack(dev, oracle, shape, side, f, dtype)
        assert len(np.unique(packed)) == packed.size


# ---- 6. staged reductions ----------------------------------------------------------------------------------------------------

REDUCTION_SHAPES = ["T1", "T2", "T4", "W1"]


def cell_index(shape, pos):
    nx, _ny, g = shape
    return (pos[1] + g) * (nx + 2 * g) + pos[0] + g


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", REDUCTION_SHAPES)
def test_dtCFL_of_a_long_block_is_the_oracles_minimum(dev, oracle, name, dtype):
    """dtCFL on the random state, then with the decisive cell (|u| = 8 where every other |u| + c is below 3) planted in row 0,
    65534, 65535, 65536, ny - 1 (T2: also 262140, 262143) or, on W1, column 0, 119, 120, 299999, nx - 1: the oracle's minimum,
    exactly (a minimum does not depend on the order). T2 takes 9 rows per workgroup, one workgroup across (gx = 1). A NaN
    in the last row gives a NaN (the reference's reduction ends in `Invalid time step` there)."""
    import armon_amd
    nx, ny, g = shape = SHAPES[name]
    T = np.dtype(dtype).type
    cflt = C.c_float if dtype == "float32" else C.c_double
    f = staged_state(nx, ny, g, dtype, 9, names=("u", "v", "c"))
    d = {k: dev.from_host(a) for k, a in f.items()}
    r = oracle.domain_range(nx, ny, g)
    size = float(T(1.) / T(nx))
    OL, fn = oracle.lib(f32=dtype == "float32"), entry(armon_amd.lib(), "dtCFL", dtype)

    def on_device(u, sizes):
        d["u"].copy_from_host(u)
        out = cflt()
        assert fn(dev.ctx, conv(r), *sizes, *(C.c_void_p(d[k].ptr) for k in ("u", "v", "c")), C.byref(out)) == 0
        return out.value

    def both(u, what, sizes=(size, size)):
        want = OL.armon_oracle_dtCFL(r, *sizes, oracle.ptr(u), oracle.ptr(f["v"]), oracle.ptr(f["c"]))
        got = on_device(u, sizes)
        assert got == want, f"{what}: {got!r} != {want!r}"
        return want

    assert np.isfinite(both(f["u"], "random state, the cell sizes of the unit square", (size, float(T(1.) / T(ny)))))
    plain = both(f["u"], "random state")                   # the same size both ways: the fastest cell decides, along or across
    assert np.isfinite(plain)
    for pos in positions(name):
        u = f["u"].copy()
        u[cell_index(shape, pos)] = T(-8.)
        planted = both(u, f"fast cell at {pos}")
        assert planted < plain and planted == T(size) / (T(8.) + f["c"][cell_index(shape, pos)])   # that cell decides
    u = f["u"].copy()
    u[cell_index(shape, (nx - 1, ny - 1))] = np.nan
    assert np.isnan(on_device(u, (size, size))), "NaN in the last row"      # (the comparisons of the oracle need not keep a NaN: no reference)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", REDUCTION_SHAPES)
def test_conservation_vars_of_a_long_block_counts_every_cell_once(dev, oracle, name, dtype):
    """rho = E = 0 except one cell with rho = 3, E = 2, at the positions of the CFL tests: whatever the order of the sums, the
    mass is exactly 3 ds and the energy exactly 6 ds with ds a power of two, in both precisions. (A row that the capped grid
    dropped, or counted twice, shows here when it holds the cell.) The same cell in a ghost row next to it counts for nothing."""
    import armon_amd
    nx, ny, g = shape = SHAPES[name]
    cflt = C.c_float if dtype == "float32" else C.c_double
    n = (nx + 2 * g) * (ny + 2 * g)
    rho, E = dev.zeros(n, dtype), dev.zeros(n, dtype)
    r = conv(oracle.domain_range(nx, ny, g))
    fn = entry(armon_amd.lib(), "conservation_vars", dtype)
    ds = 2.0 ** -20
    host = np.zeros(n, dtype=dtype)
    for pos, want in [(p, (3 * ds, 6 * ds)) for p in positions(name)] + [((0, -1), (0., 0.)), ((nx - 1, ny), (0., 0.))]:
        i = cell_index(shape, pos)
        for a, value in ((rho, 3.), (E, 2.)):
            host[i] = value
            a.copy_from_host(host)
        host[i] = 0.
        out = (cflt * 2)(-1., -1.)
        assert fn(dev.ctx, r, ds, C.c_void_p(rho.ptr), C.c_void_p(E.ptr), C.byref(out)) == 0
        assert tuple(out) == want, f"cell {pos}: (mass, energy) = {tuple(out)}, not {want}"


@pytest.mark.parametrize("name", REDUCTION_SHAPES)
def test_conservation_vars_of_a_long_block_on_a_random_state(dev, oracle, name):
    """fp64, random state, against math.fsum (the correctly rounded sum) of the addends rho and fl(rho E) over the real cells.
    A sum of n terms in ANY order is within (n - 1) eps / (1 - (n - 1) eps) times the sum of the absolute addends (Higham,
    Accuracy and Stability of Numerical Algorithms, section 4.2), and ds is a power of two, so the scaling is exact: nothing
    measured enters the bound. It is loose, but one dropped row is 4e-6 of the sum and more."""
    import armon_amd
    nx, ny, g = SHAPES[name]
    f = staged_state(nx, ny, g, "float64", 12, names=("rho", "E"))
    d = {k: dev.from_host(a) for k, a in f.items()}
    r = conv(oracle.domain_range(nx, ny, g))
    ds = 2.0 ** -20
    out = (C.c_double * 2)()
    assert armon_amd.lib().armon_hip_conservation_vars(dev.ctx, r, ds, C.c_void_p(d["rho"].ptr), C.c_void_p(d["E"].ptr), C.byref(out)) == 0
    rho = oracle.real_view(f["rho"], nx, ny, g).ravel()
    addends = rho, rho * oracle.real_view(f["E"], nx, ny, g).ravel()          # all positive: they are their absolute values
    n, eps = nx * ny, float(np.finfo(np.float64).eps)
    gamma = (n - 1) * eps / (1 - (n - 1) * eps)
    for got, terms, what in zip(out, addends, ("mass", "energy")):
        want = math.fsum(terms.tolist())
        print(f"\n{name} {what}: {abs(got / ds - want) / want:.3e} of the sum, bound {gamma:.3e}")
        assert abs(got / ds - want) <= gamma * want, f"{what}: {got / ds!r} against {want!r}"


# ---- 7. whole runs -------------------------------------------------------------------------------------------------------------

RUNS = [("Sod_circ", (10, 262147)), ("Sedov", (300007, 5))]
NAMES = ("rho", "u", "v", "E", "p")


def gpu_run(dtype, test, N, **options):
    import armon_amd
    params = armon_amd.ArmonParameters(test=test, N=N, maxcycle=3, silent=5, return_data=True, data_type=dtype, **options)
    stats = armon_amd.armon(params)
    host = stats.data.device_to_host()
    return stats, {k: stats.data.real_view(host[k]).copy() for k in NAMES}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test,N", RUNS, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_three_cycles_on_a_long_block(oracle, test, N, dtype):
    """armon() for 3 cycles on a tall and on a wide domain: the staged and the fused-exact run give the oracle's cycles, last
    step, final time and bits of rho, u, v, E, p; the fused-tuned run stays within the tolerances of
    tests/test_gpu_random_shapes.py (fields 1e-11 / 2e-4 of the field maximum, last step 1e-12 / 1e-4 relative)."""
    nx, ny = N
    orun, f = oracle.solve(test=test, N=N, maxcycle=3, data_type=np.dtype(dtype).type)
    ref = {k: oracle.real_view(f[k], nx, ny, 4) for k in NAMES}
    assert orun.cycles == 3 and all(np.isfinite(ref[k]).all() for k in NAMES)
    for what, options in (("staged", dict(use_fused_sweep=False, exact_arithmetic=True)), ("fused exact", dict(exact_arithmetic=True))):
        stats, got = gpu_run(dtype, test, N, **options)
        assert stats.cycles == orun.cycles and stats.last_dt == orun.last_dt and stats.final_time == orun.final_time, what
        for k in NAMES:
            assert np.array_equal(bits(got[k]), bits(ref[k])), f"{what} {k}: max abs diff {np.abs(got[k] - ref[k]).max()}"
        del stats, got
    stats, got = gpu_run(dtype, test, N, exact_arithmetic=False)
    assert stats.cycles == orun.cycles
    assert abs(stats.last_dt - orun.last_dt) <= (1e-12 if dtype == "float64" else 1e-4) * orun.last_dt
    tol = 1e-11 if dtype == "float64" else 2e-4
    for k in NAMES:
        scale = max(np.abs(ref[k]).max(), 1e-300)
        assert np.abs(got[k] - ref[k]).max() <= tol * scale, f"tuned {k}: {np.abs(got[k] - ref[k]).max() / scale:.3e} of the field maximum"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test,N", RUNS, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_initial_state_of_a_long_block(oracle, test, N, dtype):
    """maxcycle = 0: every field of init_test, x and y included, ghost cells included, is the oracle's."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test
    params = armon_amd.ArmonParameters(test=test, N=N, use_fused_sweep=False, data_type=dtype, silent=5)
    grid = BlockGrid(params)
    init_test(params, grid)
    got = grid.device_to_host(names=oracle.FIELDS)
    f = oracle.alloc_fields(*N, 4, fill=np.nan, dtype=np.dtype(dtype).type)
    _run, f = oracle.solve(test=test, N=N, maxcycle=0, fields=f, data_type=np.dtype(dtype).type)
    for k in oracle.FIELDS:
        assert np.array_equal(bits(got[k]), bits(f[k])), k
