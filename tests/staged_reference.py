"""Inputs and comparisons for the tests of the staged kernels (test infrastructure: a plain helper module, no fixtures).

What the GPU tests of the staged entry points share and what has to be right before a kernel is judged by it: the random
fields at any ghost width and precision, drawn ranges whose stencils provably stay inside the arrays and which provably reach
every strip origin and wave / workgroup boundary of the x forms, states whose conservation sums are exact in any summation
order, the cells a reduction can lose, and a bit-pattern comparison. tests/test_staged_reference_host.py checks this module
against the CPU oracle alone.
"""
import random

import numpy as np

from sweep_reference import draw_state

FIELD_RANGES = dict(p=(0.1, 2.0), c=(0.5, 2.0), g=(1, 2), us=(-1, 1), ps=(0.1, 2.0),
                    work_1=(-1, 1), work_2=(-1, 1), work_3=(-1, 1), work_4=(-1, 1))
GHOSTS = (2, 3, 4, 5, 6)


def rand_fields(nx, ny, g, dtype, seed, eos="perfect_gas"):
    """The fields of test_gpu_kernels.rand_state (same bounds, same order of draws) over the whole block of ghost width ``g``,
    cast to ``dtype`` here: the oracle and the kernel see the same rounded values."""
    rng = np.random.default_rng(seed)
    n = (nx + 2 * g) * (ny + 2 * g)
    f = dict(draw_state(rng, n, "perfect_gas"))
    for k, (lo, hi) in FIELD_RANGES.items():
        f[k] = rng.uniform(lo, hi, n)
    if eos == "bizarrium":
        f.update(draw_state(rng, n, "bizarrium"))
    return {k: np.ascontiguousarray(a.astype(dtype)) for k, a in f.items()}


class Precision:
    """The staged entry points of one working precision on both sides: ``hip(name)`` of the library ``L`` (``armon_hip_<name>``
    or ``armon_hip_<name>_f32``) and ``ref(name)`` of the oracle build of the same precision, run on one thread."""

    def __init__(self, L, dtype):
        import ctypes
        from oracle import oracle as O
        self.dtype = np.dtype(dtype).type
        self.f32 = self.dtype == np.float32
        self.L, self.OL = L, O.lib(f32=self.f32)
        self.OL.armon_oracle_set_threads(1)
        self.real = ctypes.c_float if self.f32 else ctypes.c_double

    def hip(self, name):
        return getattr(self.L, "armon_hip_" + name + ("_f32" if self.f32 else ""))

    def ref(self, name):
        return getattr(self.OL, "armon_oracle_" + name)


def as_tuple(r):
    return (r.col_start, r.col_step, r.col_len, r.row_start, r.row_len)


def conv(r):
    """oracle.Range → the library's Range (same layout)."""
    from armon_amd._lib import Range
    return Range(*as_tuple(r))


# ---- drawn ranges ---------------------------------------------------------------------------------------------------------
def x_form_layout(dtype):
    """(cells per 64-B sector, results per wave, results per workgroup) of the x forms of acoustic_GAD and
    advection_second_order: a wave stores 64 - S results with S/2 halo lanes on either side, a workgroup has 4 waves."""
    per_sector = 64 // np.dtype(dtype).itemsize
    wave = 64 - per_sector
    return per_sector, wave, 4 * wave


def range_of(nx, ny, g, lo, hi, axis):
    """(col_start, col_step, col_len, row_start, row_len) of the range of a drawn case: every real cell across ``axis``, real
    coordinates lo .. n - 1 + hi along it (block_domain_range with the corner offsets (lo, 0), (hi, 0) or (0, lo), (0, hi))."""
    row = nx + 2 * g
    if axis == 0:
        return (g * row, row, ny, g + lo, nx - lo + hi)
    return ((g + lo) * row, row, ny - lo + hi, g, nx)


def strip_origin(nx, ny, g, lo, hi, axis, dtype):
    """``(col_start + row_start) & (S - 1)``: where in its 64-B sector the first cell of the range sits, which is what the x
    forms shift their strips by and size their grid from."""
    col_start, _step, _len, row_start, _row_len = range_of(nx, ny, g, lo, hi, axis)
    return (col_start + row_start) & (x_form_layout(dtype)[0] - 1)


def assert_stencil_inside(nx, ny, g, lo, hi, axis):
    """The cells [i - 2s, i + 2s] of every cell i of the range lie inside the arrays, and the range is not empty."""
    col_start, col_step, col_len, row_start, row_len = range_of(nx, ny, g, lo, hi, axis)
    n = (nx + 2 * g) * (ny + 2 * g)
    s = 1 if axis == 0 else col_step
    assert nx >= 1 and ny >= 1 and col_len >= 1 and row_len >= 1, (nx, ny, g, lo, hi, axis)
    assert -2 <= lo and hi <= 2 and lo >= -(g - 2) and hi <= g - 2, (g, lo, hi)
    first = col_start + row_start
    last = col_start + (col_len - 1) * col_step + row_start + row_len - 1
    assert first - 2 * s >= 0 and last + 2 * s < n, (nx, ny, g, lo, hi, axis)
    if axis == 0:          # ... and inside their own row: a stencil that wraps into a neighbouring row reads the wrong cells
        assert row_start - 2 >= 0 and row_start + row_len - 1 + 2 < col_step, (nx, g, lo, hi)


def assert_range_coverage(cases, dtype):
    """The x-axis cases between them start on every position of a sector, and have rows shorter and longer than one wave's,
    one workgroup's and two workgroups' results."""
    per_sector, wave, group = x_form_layout(dtype)
    xs = [c for c in cases if c[5] == 0]
    origins = {strip_origin(*c[:6], dtype) for c in xs}
    assert origins == set(range(per_sector)), sorted(set(range(per_sector)) - origins)
    lengths = [range_of(*c[:6])[4] for c in xs]
    for edge in (wave, group, 2 * group):
        assert any(n < edge for n in lengths) and any(n > edge for n in lengths), edge


def draw_range_cases(seed, count, dtype):
    """``count`` cases (nx, ny, g, lo, hi, axis, limiter, seed) for acoustic_GAD and advection_second_order: a block of nx × ny
    real cells with ghost width g, and the range of every real cell across ``axis`` from real coordinate ``lo`` to ``n - 1 + hi``
    along it — first and last cell anywhere the stencil [i - 2s, i + 2s] allows: -2 <= lo, hi <= 2, and never closer than two
    cells to the edge of the arrays (lo >= -(g - 2), hi <= g - 2). The block is up to 600 cells long along the sweep and up to
    90 across it, as the ranges of test_gpu_kernels._random_flux_cases.

    The first S cases (S = cells per 64-B sector: 16 in fp32, 8 in fp64) run along x and are drawn until case k starts on
    position k of its sector, with row lengths cycling through the four classes that the results of one wave, of one workgroup
    and of two workgroups separate; the rest are free draws. Both properties are asserted on what was drawn."""
    per_sector, wave, group = x_form_layout(dtype)
    assert count >= per_sector, f"{count} cases cannot reach the {per_sector} strip origins"
    rng = random.Random(seed)
    classes = [(1, wave - 1), (wave + 1, group - 1), (group + 1, 2 * group - 1), (2 * group + 1, 600)]

    def draw(axis, length_range):
        g = rng.choice(GHOSTS)
        n_along, n_across = rng.randint(*length_range), rng.randint(1, 90)
        lo = rng.randint(max(-2, -(g - 2)), min(3, n_along - 1))
        hi = rng.randint(-min(3, n_along - 1 - max(lo, 0)), min(2, g - 2))
        nx, ny = (n_along, n_across) if axis == 0 else (n_across, n_along)
        return (nx, ny, g, lo, hi, axis, rng.randint(0, 2), rng.randint(0, 10 ** 6))

    cases = []
    for k in range(count):
        if k >= per_sector:
            cases.append(draw(rng.randint(0, 1), (1, 600)))
            continue
        lo_len, hi_len = classes[k % 4]
        for _ in range(10000):
            c = draw(0, (lo_len + 3, hi_len - 3))          # the row of the range is nx - lo + hi cells: within 3 of nx
            if strip_origin(*c[:6], dtype) == k and lo_len <= range_of(*c[:6])[4] <= hi_len:
                cases.append(c)
                break
        else:
            raise AssertionError(f"no case found for strip origin {k}")
    for c in cases:
        assert_stencil_inside(*c[:6])
    assert_range_coverage(cases, dtype)
    return cases


# ---- exact sums -----------------------------------------------------------------------------------------------------------
def dyadic_state(nx, ny, g, dtype, seed):
    """(rho, E, ds): rho in {1/8 .. 16/8}, E in {1/4 .. 16/4} over the whole ghosted block, ds a power of two. Every rho is a
    multiple of 1/8 and every product rho·E a multiple of 1/32, so every partial sum of them, in any order, is such a multiple
    too, and it is exact in fp32 while it stays below 2^24 of these units. The bound is asserted for the worst state of the
    shape with one cell of rho raised by 1/8 (what the tests do to it): nx·ny·(17/8 · 4)·32 < 2^24."""
    assert nx * ny * 17 * 16 < 2 ** 24, f"{nx} x {ny}: the sums of rho·E may need more than 24 bits"
    rng = np.random.default_rng(seed)
    n = (nx + 2 * g) * (ny + 2 * g)
    rho = (rng.integers(1, 17, n) / 8.).astype(dtype)
    E = (rng.integers(1, 17, n) / 4.).astype(dtype)
    ds = np.dtype(dtype).type(2.) ** int(-rng.integers(3, 13))
    return rho, E, ds


def real_view(a, nx, ny, g):
    return a.reshape(ny + 2 * g, nx + 2 * g)[g:g + ny, g:g + nx]


def exact_sums(rho, E, ds, nx, ny, g):
    """(mass, energy) of the real cells in float64: exact for a ``dyadic_state``."""
    r = real_view(rho, nx, ny, g).astype(np.float64)
    e = real_view(E, nx, ny, g).astype(np.float64)
    return float(np.sum(r) * float(ds)), float(np.sum(r * e) * float(ds))


# ---- where a reduction can lose a cell ------------------------------------------------------------------------------------
def EXTREME_POSITIONS(nx, ny):
    """Real cells (what, row, column), 0-based, that a two-cells-per-lane reduction over groups of four rows can lose: the
    corners; the last cell of an odd row (the one no pair holds); both halves of the first and of the last pair of a row; the
    cells on either side of the first 512 of a row (one pass of a workgroup's 256 lanes); the first and last row of the last,
    partial group of four rows. Each cell is listed once, under the first name it gets."""
    mid_row, mid_col = ny // 2, nx // 2
    pos = [("first cell of the first row", 0, 0), ("last cell of the first row", 0, nx - 1),
           ("first cell of the last row", ny - 1, 0), ("last cell of the last row", ny - 1, nx - 1)]
    if nx % 2:
        pos.append(("odd tail of a row", mid_row, nx - 1))
    if nx >= 2:
        last_pair = 2 * (nx // 2 - 1)
        pos += [("first pair .x", mid_row, 0), ("first pair .y", mid_row, 1),
                ("last pair .x", mid_row, last_pair), ("last pair .y", mid_row, last_pair + 1)]
    pos += [(f"cell {k} of a row", mid_row, k) for k in (511, 512, 513) if k < nx]
    if ny % 4:
        pos += [("first row of the last group of rows", 4 * (ny // 4), mid_col), ("last row of the last group of rows", ny - 1, mid_col)]
    seen, out = set(), []
    for what, row, col in pos:
        assert 0 <= row < ny and 0 <= col < nx
        if (row, col) not in seen:
            seen.add((row, col))
            out.append((what, row, col))
    return out


def flat_index(nx, g, row, col):
    """Index in the flat ghosted array of the real cell (row, col)."""
    return (row + g) * (nx + 2 * g) + col + g


PLANTED = -7.3          # a velocity no cell of rand_fields comes near: |u| + c < 3 there


def cfl_closed_form(d, vel, c):
    """``d / (|vel| + |c|)`` in the precision of ``c``: the CFL step of the one cell that decides the reduction."""
    T = np.asarray(c).dtype.type
    with np.errstate(all="ignore"):
        return T(d) / (abs(T(vel)) + abs(T(c)))


# ---- bit patterns ---------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits_equal(got, want, name, pitch=None, rng=None):
    """``got`` and ``want`` hold the same bit patterns (NaN payloads and the sign of zero count). With the row ``pitch`` of
    the arrays the first difference is reported as (row, column), and with ``rng`` = (col_start, col_step, col_len, row_start,
    row_len) also as inside / outside that range."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    diff = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    if diff.size == 0:
        return
    i = int(diff[0])
    where = f"index {i}"
    if pitch:
        where = f"(row {i // pitch}, column {i % pitch})"
        if rng is not None:
            col_start, col_step, col_len, row_start, row_len = rng
            j, k = divmod(i - col_start - row_start, col_step) if col_step else (0, i - col_start - row_start)
            inside = 0 <= j < col_len and 0 <= k < row_len
            where += " inside the range" if inside else " OUTSIDE the range"
    g, w = got.ravel()[i], want.ravel()[i]
    raise AssertionError(f"{name}: {diff.size} cells differ, first at {where}: got {g!r} ({int(bits(got).ravel()[i]):#x}), "
                         f"want {w!r} ({int(bits(want).ravel()[i]):#x})")
