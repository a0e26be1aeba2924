"""Mixing measures on the GPU: armon_hip_mixing / armon_hip_mixing_bounds / armon_hip_scalar_pdf and the Python surface over
them (BlockGrid.mixing, BlockGrid.scalar_pdf, the mixing_* options).

The oracle is mixing.reference_record / reference_bounds / reference_pdf applied to the planes the test uploaded. Everything is
compared WORD FOR WORD, never within a tolerance: every addend is rounded once to an integer and integer sums have no order.
The ghosts of every input hold NaN: a ghost that is read shows as a bad cell.

The thresholds of the kernels: a span is 128 (fp64) or 256 (fp32) columns, a tile 32 rows of which a wave
takes 8; the LDS table holds 264 bins; a workgroup walks more than one tile once the window has more tiles than the grid has
workgroups (the cap PROFILE_WGS brings that within reach of a small window; the two long blocks cross it uncapped)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
NAMES = ("a", "b", "c", "d")
N = (264, 70)
# (wnx, wny): each side of a span in both types, of a wave's 8 rows, of a tile's 32 rows, two tiles and a row; the smallest windows
SHAPES = [(127, 7), (128, 8), (129, 9), (255, 31), (256, 32), (257, 33), (129, 65), (1, 1), (1, 7), (7, 1), (260, 67)]
# (axis, width, bins): a span's worth of bins, a bin per row, bins that span tiles, one bin, bins that cut cells off
CONFIGS = [("x", 1, None), ("y", 1, None), ("x", 3, None), ("y", 3, None), ("x", 50, None), ("y", 50, None), ("x", 1000, None),
           ("y", 1000, None), ("x", 3, 9), ("y", 1, 5)]

_grids = {}


def A():
    import armon_amd
    return armon_amd


def planted(N, dtype, nghost=None, ns=4, seed=1):
    """A block whose rho and ``ns`` scalar planes hold random real cells — rho in [0.1, 10], φ in [-0.5, 1.5] — and NaN in
    every ghost → (grid, dict name → the (ny, nx) real cells as uploaded)."""
    from armon_amd.solver import BlockGrid
    key = (N, dtype, nghost, ns, seed)
    if key not in _grids:
        kw = {} if nghost is None else dict(nghost=nghost)
        params = A().ArmonParameters(test="Sod", N=N, data_type=dtype, silent=5, scalars=[A().Scalar(n) for n in NAMES[:ns]], **kw)
        grid = BlockGrid(params)
        rng = np.random.default_rng(seed)
        real = {}
        for name, (lo, hi) in [("rho", (0.1, 10.0))] + [(n, (-0.5, 1.5)) for n in NAMES[:ns]]:
            full = np.full((grid.size.size[1], grid.size.size[0]), np.nan, dtype=dtype)
            grid.real_view(full)[...] = rng.uniform(lo, hi, (N[1], N[0])).astype(dtype)
            grid.data[name if name == "rho" else "s:" + name].copy_from_host(full.ravel())
            real[name] = grid.real_view(full).copy()
        _grids[key] = (grid, real)
    return _grids[key]


@pytest.fixture(scope="module", autouse=True)
def release_grids():
    yield
    _grids.clear()


def set_wgs(grid, n):
    dev = grid.params.device
    assert dev._L.armon_hip_set_tuning(dev.ctx, b"PROFILE_WGS", int(n)) == 0


def cut(a, window):
    col0, row0, wnx, wny = window
    return a[row0:row0 + wny, col0:col0 + wnx]


def same_words(P, want, what):
    got = P.raw
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        b, w = bad[0]
        raise AssertionError(f"{what}: {len(bad)} words differ, first in bin {b} word {w}: {int(got[b, w]):#x} != {int(want[b, w]):#x}")
    assert not got[:, 19:].any()                                       # the reserved word stays zero


def check_window(grid, real, window, axis, width, bins, names, what):
    """The device's profiles of ``window`` under the default scale against the restatement; the bounds against its own."""
    from armon_amd import mixing as mix
    tiles = [(grid.params, grid)]
    out = mix.mixing_state(tiles, axis, width=width, scalars=names, windows=[window], bins=bins)
    spec = mix.make_spec(grid.params, axis, width, bins)
    bounds = mix.state_bounds(tiles, spec, names, [window])
    rho = cut(real["rho"], window)
    cells = 0
    for k, name in enumerate(names):
        P, phi = out[name], cut(real[name], window)
        assert bounds[k] == mix.reference_bounds(rho, phi), (what, name)
        assert P.scale_exp == mix.default_scale(bounds[k])
        same_words(P, mix.reference_record(axis, P.nbins, width, P.scale_exp, rho, phi, origin=window[:2]), (what, name))
        assert int(P.n_bad.sum()) == 0, (what, name)                   # the default scale refuses no cell, and no ghost was read
        cells = int(P.n.sum())
        assert cells == window[2] * window[3] or bins is not None
    return out, cells


@pytest.mark.parametrize("nghost", [4, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_word_for_word_at_every_threshold(dtype, nghost):
    """Rows of 264 + 2 nghost cells. nghost 4 (pitch 272): col0 = 0 takes the 16-B loads in both types, col0 = 3 the element
    loads. nghost 5 (pitch 274): col0 = 3 takes the 16-B loads in fp64 (the window's first cell is even), everything else the
    element loads."""
    grid, real = planted(N, dtype, nghost)
    set_wgs(grid, 0)
    for wnx, wny in SHAPES:
        for col0, row0 in ((0, 0), (3, 2)):
            for axis, width, bins in CONFIGS:
                window = (col0, row0, wnx, wny)
                check_window(grid, real, window, axis, width, bins, ("c",), (dtype, nghost, window, axis, width, bins))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_whole_block_and_a_capped_grid_change_no_word(dtype):
    """3 workgroups for 3 x 3 (fp64) or 2 x 3 (fp32) tiles: every workgroup walks several tiles, the table's base changes inside
    its run (x: with the span, y: with the row block), and the words are those of the uncapped launch."""
    from armon_amd import mixing as mix
    grid, real = planted(N, dtype, 4)
    whole = (0, 0) + N
    for axis, width in (("x", 1), ("y", 1), ("x", 7), ("y", 7)):
        set_wgs(grid, 0)
        free, cells = check_window(grid, real, whole, axis, width, None, NAMES, (dtype, axis, width))
        assert cells == N[0] * N[1]
        assert free == grid.mixing(axis, width)                        # the public call is this one
        for cap in (1, 3):
            set_wgs(grid, cap)
            try:
                capped = grid.mixing(axis, width)
            finally:
                set_wgs(grid, 0)
            assert capped == free and all(np.array_equal(capped[n].raw, free[n].raw) for n in NAMES), (dtype, axis, width, cap)
    # a global position that is not the window's own: bins by the global cell
    (P,) = mix.mixing_state([(grid.params, grid)], "y", width=4, scalars=("b",), windows=[(5, 13, 100, 40)]).values()
    assert P.n.tolist()[:3] == [0, 0, 0] and P.n[3] == 300 and P.n[4] == 400 and int(P.n.sum()) == 4000


@pytest.mark.parametrize("dtype", DTYPES)
def test_four_planes_in_one_call_are_four_calls_and_bad_cells_stay_in_their_plane(dtype):
    from armon_amd import mixing as mix
    grid, real = planted(N, dtype, 4)
    tiles = [(grid.params, grid)]
    scales = {n: (-70 - k,) * 5 for k, n in enumerate(NAMES)}
    for axis in "xy":
        four = mix.mixing_state(tiles, axis, width=2, scale_exp=scales)
        for n in NAMES:
            (one,) = mix.mixing_state(tiles, axis, width=2, scalars=(n,), scale_exp={n: scales[n]}).values()
            assert one == four[n] and np.array_equal(one.raw, four[n].raw), (axis, n)
            same_words(one, mix.reference_record(axis, one.nbins, 2, scales[n], real["rho"], real[n]), (axis, n))
    # a NaN and an inf planted in plane c: its n_bad rises, the other three planes keep every word
    before = mix.mixing_state(tiles, "y", scale_exp=scales)
    plane = grid.data["s:c"]
    saved = plane.to_host()
    try:
        full = saved.copy().reshape(grid.size.size[1], grid.size.size[0])
        view = grid.real_view(full)
        view[11, 17], view[40, 200] = np.nan, np.inf
        plane.copy_from_host(full.ravel())
        after = mix.mixing_state(tiles, "y", scale_exp=scales)
        for n in "abd":
            assert np.array_equal(after[n].raw, before[n].raw), n
        assert after["c"].n_bad.tolist() == [1 if r in (11, 40) else 0 for r in range(N[1])]
        assert (before["c"].n - after["c"].n).tolist() == after["c"].n_bad.tolist()
        same_words(after["c"], mix.reference_record("y", N[1], 1, scales["c"], real["rho"], view), "planted")
        bounds = mix.state_bounds(tiles, mix.make_spec(grid.params, "y"), ("c",))
        assert bounds[0] == mix.reference_bounds(real["rho"], view)     # the bounds pass skips what is not finite
    finally:
        plane.copy_from_host(saved)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_window_split_2x2_merges_to_the_whole(dtype):
    from armon_amd import mixing as mix
    grid, real = planted(N, dtype, 5)
    tiles = [(grid.params, grid)]
    scales = [(-72,) * 5] * 4
    for axis, width in (("x", 1), ("y", 3)):
        whole = mix.mixing_state(tiles, axis, width=width, scale_exp=scales)
        merged = None
        for row0, wny in ((0, 33), (33, 37)):
            for col0, wnx in ((0, 129), (129, 135)):
                part = mix.mixing_state(tiles, axis, width=width, scale_exp=scales, windows=[(col0, row0, wnx, wny)])
                merged = part if merged is None else {n: merged[n].merge(part[n]) for n in NAMES}
        for n in NAMES:
            assert np.array_equal(merged[n].raw, whole[n].raw), (axis, n)


@pytest.mark.parametrize("shape,dtype", [((300007, 3), "float64"), ((3, 70001), "float32")], ids=["long_rows", "many_rows"])
def test_blocks_with_more_tiles_than_workgroups(shape, dtype):
    """2344 spans of one row block, and 2188 row blocks of one span: more tiles than any grid has workgroups."""
    grid, real = planted(shape, dtype, ns=1, seed=2)
    set_wgs(grid, 0)
    whole = (0, 0) + shape
    for axis, width in (("x", 1), ("y", 1), ("x", 50), ("y", 50)):
        _, cells = check_window(grid, real, whole, axis, width, None, ("a",), (shape, axis, width))
        assert cells == shape[0] * shape[1]
    from armon_amd import mixing as mix
    P = grid.scalar_pdf("a", bins=64, range=(-0.5, 1.5))
    want = mix.reference_pdf(real["rho"], real["a"], -0.5, mix.inv_width(-0.5, 1.5, 64), 64, P.rho_scale_exp)
    assert np.array_equal(P.raw, want) and int(P.counts.sum()) == shape[0] * shape[1]


def test_the_c_abi_refusals_write_nothing():
    from armon_amd._lib import MixingSpec, PdfSpec
    grid, _ = planted(N, "float64", 4)
    params, dev = grid.params, grid.params.device
    L = dev._L
    pattern = np.arange(1, 4 * 70 * 20 + 1, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)
    out = dev.from_host(pattern)
    try:
        spec = MixingSpec()
        spec.axis, spec.nbins, spec.width = 1, 70, 1
        planes = (C.c_void_p * 4)(*[grid.data["s:" + n].ptr for n in NAMES])
        rho = C.c_void_p(grid.data["rho"].ptr)

        def call(fn, ns=4, phi=planes, spec=spec, wnx=N[0], col0=0, gcol=0, out_ptr=None, rho=rho):
            return fn(dev.ctx, grid.size.size[0], grid.size.ghosts, N[0], N[1], rho, ns, phi, col0, 0, wnx, N[1], gcol, 0,
                      C.byref(spec), C.c_void_p(out.ptr) if out_ptr is None else out_ptr)

        bad_axis, bad_scale, bad_bins = MixingSpec(), MixingSpec(), MixingSpec()
        for s, (axis, nbins, width) in ((bad_axis, (2, 70, 1)), (bad_scale, (1, 70, 1)), (bad_bins, (1, 0, 1))):
            s.axis, s.nbins, s.width = axis, nbins, width
        bad_scale.scale_exp[3][4] = 4097
        holed = (C.c_void_p * 4)(planes[0], planes[1], planes[2], None)
        for fn in (L.armon_hip_mixing, L.armon_hip_mixing_bounds):
            for kw in (dict(ns=0), dict(ns=5), dict(phi=holed), dict(phi=None), dict(rho=None), dict(spec=bad_axis), dict(spec=bad_scale),
                       dict(spec=bad_bins), dict(wnx=N[0] + 1), dict(col0=1), dict(gcol=-1)):
                assert call(fn, **kw) == 1, kw                         # the last plane's fault is found before the first plane is launched
        assert L.armon_hip_mixing_reset(dev.ctx, 5, 70, C.c_void_p(out.ptr)) == 1
        assert L.armon_hip_mixing_reset(dev.ctx, 4, 0, C.c_void_p(out.ptr)) == 1
        pdf = PdfSpec()
        pdf.lo, pdf.inv_w, pdf.nbins, pdf.rho_scale_exp = 0.0, 64.0, 64, -60
        for field, value in (("nbins", 0), ("nbins", 1025), ("inv_w", 0.0), ("inv_w", math.inf), ("lo", math.nan), ("rho_scale_exp", 5000)):
            bad = PdfSpec()
            bad.lo, bad.inv_w, bad.nbins, bad.rho_scale_exp = pdf.lo, pdf.inv_w, pdf.nbins, pdf.rho_scale_exp
            setattr(bad, field, value)
            assert L.armon_hip_scalar_pdf(dev.ctx, grid.size.size[0], grid.size.ghosts, N[0], N[1], rho, planes[0], 0, 0, N[0], N[1],
                                          C.byref(bad), C.c_void_p(out.ptr)) == 1, (field, value)
        assert L.armon_hip_scalar_pdf(dev.ctx, grid.size.size[0], grid.size.ghosts, N[0], N[1], rho, planes[0], 0, 0, N[0], N[1] + 1,
                                      C.byref(pdf), C.c_void_p(out.ptr)) == 1
        assert L.armon_hip_scalar_pdf_reset(dev.ctx, 1025, C.c_void_p(out.ptr)) == 1
        params.wait()
        assert np.array_equal(out.to_host(), pattern)
        # and what is accepted starts from what is there: a pass over records that were not reset merges into them
        assert L.armon_hip_mixing_reset(dev.ctx, 4, 70, C.c_void_p(out.ptr)) == 0
        params.wait()
        from armon_amd import mixing as mix
        assert np.array_equal(out.to_host().reshape(4, 70, 20), np.stack([mix.neutral(70)] * 4))
    finally:
        out.free()


# ---- the histogram ---------------------------------------------------------------------------------------------------------
def with_plane(grid, name, values, fill):
    """Context: the first cells of the real domain of the plane ``name`` hold ``values``, the rest ``fill``."""
    class Planted:
        def __enter__(self):
            plane = grid.data["s:" + name]
            self.saved = plane.to_host()
            full = self.saved.copy().reshape(grid.size.size[1], grid.size.size[0])
            view = grid.real_view(full)
            flat = np.full(view.size, fill, dtype=full.dtype)
            flat[:len(values)] = values
            view[...] = flat.reshape(view.shape)
            plane.copy_from_host(full.ravel())
            return view.copy()

        def __exit__(self, *exc):
            grid.data["s:" + name].copy_from_host(self.saved)
            return False
    return Planted()


def pdf_words_of(grid, real_rho, phi, name, bins, rng, **kw):
    from armon_amd import mixing as mix
    P = grid.scalar_pdf(name, bins=bins, range=rng, **kw)
    window = kw.get("window") or (0, 0) + tuple(grid.params.N)
    want = mix.reference_pdf(cut(real_rho, window), cut(phi, window), rng[0], mix.inv_width(rng[0], rng[1], bins), bins, P.rho_scale_exp)
    assert np.array_equal(P.raw, want), (name, bins, rng, kw, np.flatnonzero(P.raw != want)[:8])
    assert int(P.counts.sum()) + P.below[0] + P.above[0] + P.bad == window[2] * window[3]
    return P


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_histogram_at_its_edges(dtype):
    grid, real = planted(N, dtype, 4)
    set_wgs(grid, 0)
    edges = np.arange(65) / 64                                        # exact in both types
    e, inf = edges.astype(dtype), np.array(np.inf, dtype=dtype)
    values = np.concatenate([e, np.nextafter(e, -inf), np.nextafter(e, inf), np.array([-0.0, np.nan, np.inf, -np.inf], dtype=dtype)])
    assert values.dtype == np.dtype(dtype)
    with with_plane(grid, "a", values, 0.5) as phi:
        P = pdf_words_of(grid, real["rho"], phi, "a", 64, (0.0, 1.0))
        others = N[0] * N[1] - len(values)
        want = np.full(64, 3)
        want[0] += 1                                                  # -0.0 is not below 0.0
        want[32] += others
        assert P.counts.tolist() == want.tolist() and P.below[0] == 1 and P.above[0] == 2 and P.bad == 3
        for bins, rng in ((10, (0.0, 1.0)), (1, (0.0, 1.0)), (2, (0.0, 1.0)), (1024, (0.0, 1.0)), (7, (-0.3, 1.1))):
            pdf_words_of(grid, real["rho"], phi, "a", bins, rng)
    # the random plane: every lane changes its bin at nearly every cell; windows on both alignment paths; a split that merges
    for bins in (1, 2, 64, 1024):
        whole = pdf_words_of(grid, real["rho"], real["b"], "b", bins, (-0.5, 1.5))
        assert whole.bad == 0 and int(whole.counts.sum()) == N[0] * N[1]
    for window in ((0, 0, 128, 8), (3, 2, 129, 9), (2, 1, 257, 33), (0, 0, 1, 1), (1, 0, 1, 7), (0, 3, 7, 1)):
        pdf_words_of(grid, real["rho"], real["b"], "b", 64, (0.0, 1.0), window=window)
    from armon_amd import mixing as mix
    s = whole.rho_scale_exp
    parts = [mix.pdf_state([(grid.params, grid)], "b", bins=16, range=(0.0, 1.0), rho_scale_exp=s, windows=[w])
             for w in ((0, 0, 129, 33), (129, 0, 135, 33), (0, 33, 129, 37), (129, 33, 135, 37))]
    merged = parts[0].merge(parts[1]).merge(parts[2]).merge(parts[3])
    assert merged == mix.pdf_state([(grid.params, grid)], "b", bins=16, range=(0.0, 1.0), rho_scale_exp=s)
    for cap in (1, 3):                                                # the cap on the workgroups changes no word
        set_wgs(grid, cap)
        try:
            assert mix.pdf_state([(grid.params, grid)], "b", bins=16, range=(0.0, 1.0), rho_scale_exp=s) == merged
        finally:
            set_wgs(grid, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_field_that_is_0_or_1_almost_everywhere(dtype):
    """Every lane stays in one of two bins for long runs, and all lanes hit the same two rows of the table."""
    grid, real = planted(N, dtype, 5)
    values = np.where(np.arange(N[0] * N[1]) < N[0] * 35, 0.0, 1.0).astype(dtype)
    values[[5, 9000, 9001, 18000]] = [0.25, 0.5, 0.75, 0.999]
    with with_plane(grid, "d", values, 1.0) as phi:
        P = pdf_words_of(grid, real["rho"], phi, "d", 64, (0.0, 1.0))
        assert P.counts[0] == N[0] * 35 - 3 and P.above[0] == N[0] * 35 - 1 and P.counts[16] == P.counts[32] == P.counts[48] == P.counts[63] == 1
        P = pdf_words_of(grid, real["rho"], phi, "d", 2, (0.0, 1.0 + 2.0 ** -20))       # 1.0 inside the range: two rows take it all
        assert P.counts.tolist() == [N[0] * 35 - 1, N[0] * 35 + 1] and P.above[0] == 0
        M = grid.mixing("y", scalars=["d"])["d"]
        assert M.extent(0.0, 1.0) is not None and M.minimum == 0.0 and M.maximum == 1.0


# ---- runs ------------------------------------------------------------------------------------------------------------------
def same_table(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


def rayleigh_taylor(**kw):
    """64 x 96, heavy over light with a tagged upper half, a perturbed interface, gravity, periodic in x."""
    nx, ny = 64, 96
    y = (np.arange(ny) + 0.5)[:, None] / ny * 1.5
    x = (np.arange(nx) + 0.5)[None, :] / nx
    front = 0.75 + 0.02 * np.cos(2 * np.pi * x)
    heavy = (y > front).astype(np.float64) * np.ones((ny, nx))
    rho = 1.0 + heavy
    p = 2.5 - 0.1 * rho * (y - 0.75)
    zero = np.zeros((ny, nx))
    problem = A().Problem.from_arrays(rho, zero, zero, p=p, boundaries=("Periodic", "Periodic", "Dirichlet", "Dirichlet"),
                                      domain_size=(1.0, 1.5), gravity=(0.0, -0.1), scalars=[A().Scalar("heavy", array=heavy)],
                                      maxtime=1e9, cfl=0.4)
    return A().ArmonParameters(test=problem, N=(nx, ny), maxcycle=20, silent=5, return_data=True, **kw)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_run_samples_writes_and_does_not_disturb(tmp_path, dtype, exact):
    from armon_amd import io as aio
    from armon_amd import mixing as mix
    base = dict(data_type=dtype, exact_arithmetic=exact, output_dir=str(tmp_path))
    plain = A().armon(rayleigh_taylor(**base))
    stats = A().armon(rayleigh_taylor(mixing_step=5, mixing_pdf_bins=16, mixing_bin_width=2, **base))
    assert [s[0] for s in stats.mixing] == [5, 10, 15, 20] and stats.cycles == 20 and plain.mixing == []
    # the run is the run without the options, bit for bit
    names = ("rho", "u", "v", "E", "s:heavy")
    assert stats.data.state_digest(names) == plain.data.state_digest(names) and stats.final_time == plain.final_time
    for n in names:
        assert np.array_equal(stats.data.data[n].to_host(), plain.data.data[n].to_host(), equal_nan=True), n
    # the files read back equal
    series = aio.read_mixing_series(str(tmp_path / "mixing.txt"))
    assert series["scalars"] == ["heavy"] and series["cycle"].tolist() == [5, 10, 15, 20]
    for i, (cycle, time, profiles, pdfs) in enumerate(stats.mixing):
        assert series["time"][i] == time and set(profiles) == set(pdfs) == {"heavy"}
        got_profiles, got_pdfs = aio.read_mixing_file(str(tmp_path / f"mixing_{cycle:06d}.txt"))
        same_table(got_profiles["heavy"], profiles["heavy"].table())
        same_table(got_pdfs["heavy"], pdfs["heavy"].table())
        m = profiles["heavy"].measures()
        for k in aio.MIXING_MEASURES:
            assert series["heavy"][k][i] == m[k] or (math.isnan(m[k]) and math.isnan(series["heavy"][k][i])), (cycle, k)
    # the last sample is the restatement of the state that is still there
    cycle, time, profiles, pdfs = stats.mixing[-1]
    grid = stats.data
    host = grid.device_to_host(("rho",))
    rho, phi = grid.real_view(host["rho"]), grid.scalar("heavy")
    P = profiles["heavy"]
    assert (P.cycle, P.axis, P.width, P.nbins) == (20, "y", 2, 48)
    assert P.scale_exp == mix.default_scale(mix.reference_bounds(rho, phi))
    assert np.array_equal(P.raw, mix.reference_record("y", 48, 2, P.scale_exp, rho, phi)) and int(P.n.sum()) == 64 * 96 and not P.n_bad.any()
    D = pdfs["heavy"]
    assert np.array_equal(D.raw, mix.reference_pdf(rho, phi, 0.0, 16.0, 16, D.rho_scale_exp)) and D.rho_scale_exp == P.scale_exp[0]
    assert int(D.counts.sum()) + D.below[0] + D.above[0] == 64 * 96 and D.bad == 0
    # the layer has a width and an extent (the content's drift is printed: the remap conserves it to rounding)
    first = stats.mixing[0][2]["heavy"]
    assert P.integral_width > 0 and math.isfinite(P.mixedness) and P.extent() is not None
    print(f"\n{dtype} {'exact' if exact else 'tuned'}: content {first.content:.15g} -> {P.content:.15g}, W = {P.integral_width:.6g}, "
          f"Theta = {P.mixedness:.6g}, extent = {P.extent()}, phi in [{P.minimum:.6g}, {P.maximum:.6g}]")


def test_a_run_with_no_step_sample_and_a_run_without_scalars(tmp_path):
    import os
    stats = A().armon(rayleigh_taylor(mixing_at_end=True, mixing_axis="x", output_dir=str(tmp_path / "end")))
    assert [s[0] for s in stats.mixing] == [20] and stats.mixing[0][3] is None and stats.mixing[0][2]["heavy"].axis == "x"
    assert sorted(os.listdir(tmp_path / "end")) == ["mixing.txt", "mixing_000020.txt"]
    stats = A().armon(rayleigh_taylor(mixing_step=50, output_dir=str(tmp_path / "none")))      # the run stops before the first sample
    assert stats.mixing == [] and not os.path.exists(tmp_path / "none")
    with pytest.raises(A().SolverException) as e:
        A().ArmonParameters(test="Sod", N=(64, 96), mixing_step=5)
    assert e.value.category == "config"
