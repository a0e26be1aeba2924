"""State comparison on the GPU: armon_hip_state_compare / armon_hip_state_diff_reset, BlockGrid / TileGroup .compare_state and
the run options over them (compare_step, compare_dir, compare_at_end, comparison_atol).

The oracle is the numpy restatement of the per-cell rule in armon_amd.compare (cell_rule / diff_reference; pinned on hand-made
pairs by tests/test_compare_host.py): every field of every record is compared bit for bit, there is no tolerance in these
tests other than the ones handed to the kernel."""
import ctypes as C
import os
import shutil
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("rho", "u", "v", "E")
NONE = (1 << 64) - 1
U64 = np.uint64
SHAPES = [(1, 1, 4), (37, 19, 3), (130, 9, 4), (256, 70, 2), (515, 33, 5)]


def _block(nx, ny, nghost, nvars, dtype, seed):
    """A bare block of ``nvars`` random vectors (ghosts included) → (params, device arrays, host copies)."""
    import armon_amd
    # the entry points take any ghost width >= 0; ArmonParameters only the ones a scheme can run with: it supplies the device
    # and the data type here, the geometry of the block is this function's own
    run_params = armon_amd.ArmonParameters(test="Sod", N=(nx, ny), data_type=dtype, silent=5)
    params = types.SimpleNamespace(device=run_params.device, fn=run_params.fn, wait=run_params.wait, N=(nx, ny), nghost=nghost)
    rng = np.random.default_rng(seed)
    n = (nx + 2 * nghost) * (ny + 2 * nghost)
    host = [rng.standard_normal(n).astype(dtype) for _ in range(nvars)]
    return params, [params.device.from_host(h) for h in host], host


def real(h, nx, ny, g):
    return h.reshape(ny + 2 * g, nx + 2 * g)[g:g + ny, g:g + nx]


def plant(ours, ref, rng):
    """Every kind of difference at drawn positions that include the four corners, the last column of a span and the first of
    the next (spans are 64 lanes x 2 or 4 columns), into the reference (and into ours where both sides take part)."""
    ny, nx = ref.shape
    span = 64 * (2 if ref.dtype.itemsize == 8 else 4)
    spots = [(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)]
    spots += [(int(rng.integers(ny)), c) for c in (span - 1, span, 2 * span - 1, 2 * span) if c < nx]
    spots += [(int(rng.integers(ny)), int(rng.integers(nx))) for _ in range(12)]
    spots = list(dict.fromkeys(spots))
    T, tiny = ref.dtype.type, np.finfo(ref.dtype).smallest_subnormal
    kinds = ["ulp", "rel", "zero", "nan_one", "nan_both", "inf_same", "inf_opposite", "subnormal"]
    turn = int(rng.integers(len(kinds)))                          # every kind once over the first spots, then drawn
    for k, (j, i) in enumerate(spots):
        kind = kinds[int(rng.integers(len(kinds)))] if k >= len(kinds) else kinds[(k + turn) % len(kinds)]
        if kind == "ulp":
            ref[j, i] = np.nextafter(ours[j, i], T(np.inf))
        elif kind == "rel":
            ref[j, i] = ours[j, i] * T(1 + 1e-3)
        elif kind == "zero":
            ours[j, i], ref[j, i] = T(0.0), T(-0.0)
        elif kind == "nan_one":
            ref[j, i] = T(np.nan)
        elif kind == "nan_both":
            ours[j, i] = ref[j, i] = T(np.nan)
        elif kind == "inf_same":
            ours[j, i] = ref[j, i] = T(np.inf)
        elif kind == "inf_opposite":
            ours[j, i], ref[j, i] = T(np.inf), T(-np.inf)
        else:
            ours[j, i], ref[j, i] = T(3) * tiny, tiny


def compare_call(params, arrays, window, gfirst, NX, ref, rtol, atol, diff, row_out=None, nvars=None, ctx=True, suffix=None):
    nvars = len(arrays) if nvars is None else nvars
    ptrs = (C.c_void_p * max(len(arrays), nvars, 1))(*[a.ptr for a in arrays])
    g = params.nghost
    ptr = lambda a: C.c_void_p(a if isinstance(a, int) else a.ptr) if a is not None else None
    return params.fn("state_compare")(params.device.ctx if ctx else None, params.N[0] + 2 * g, g, params.N[0], params.N[1], nvars,
                                      ptrs, *window, gfirst, NX, ptr(ref), rtol, atol, ptr(diff), ptr(row_out))


def reset(params, diff, nvars=8):
    assert params.device._L.armon_hip_state_diff_reset(params.device.ctx, nvars, C.c_void_p(diff.ptr)) == 0


def records(params, diff, nvars):
    params.wait()
    return [tuple(int(v) for v in r) for r in diff.to_host().reshape(8, 8)[:nvars]]


def planted_pair(nx, ny, g, dtype, seed, nvars=3):
    """→ (params, device vectors, ours real planes, reference planes [nvars][ny][nx]) with differences planted."""
    params, arrays, host = _block(nx, ny, g, nvars, dtype, seed)
    rng = np.random.default_rng(seed + 1)
    ours = [real(h, nx, ny, g) for h in host]                     # views: planting writes through to the vectors' host copies
    ref = np.stack([o.copy() for o in ours])
    for q in range(nvars):
        plant(ours[q], ref[q], rng)
    for a, h in zip(arrays, host):
        a.copy_from_host(h)
    return params, arrays, ours, ref


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_field_against_the_numpy_rule(shape, dtype):
    from armon_amd.compare import cell_rule, diff_reference
    nx, ny, g = shape
    NX, gx0, gy0 = 1000, 11, 5                                   # the block as a tile of a wider domain
    eps = float(np.finfo(dtype).eps)
    params, arrays, ours, ref = planted_pair(nx, ny, g, dtype, seed=nx * 7 + ny)
    dev = params.device
    ref_dev, diff, row_out = dev.from_host(ref.ravel()), dev.empty(64, U64), dev.empty(3 * ny, np.uint32)
    for rtol in (0.0, 4 * eps, 1e-10):
        for atol in (0.0, 1e-13):
            reset(params, diff)
            row_out.fill_bytes(0)
            assert compare_call(params, arrays, (0, 0, nx, ny), gy0 * NX + gx0, NX, ref_dev, rtol, atol, diff, row_out) == 0
            got = records(params, diff, 3)
            rows = row_out.to_host().reshape(3, ny)
            for q in range(3):
                want = diff_reference(ours[q], ref[q], rtol, atol, NX, (gx0, gy0))
                assert got[q] == want, (rtol, atol, q, dict(zip(("cells", "bits", "out", "first", "abs", "abs_at", "rel", "rel_at"), zip(got[q], want))))
                assert rows[q].tolist() == cell_rule(ours[q], ref[q], rtol, atol)[1].sum(axis=1).tolist(), (rtol, atol, q)
            assert nx * ny < 8 or (got[0][1] > 0 and got[0][2] > 0)                   # the planting took
            assert records(params, diff, 8)[3:] == [(0, 0, 0, NONE, 0, NONE, 0, NONE)] * 5       # other records untouched
    for a in arrays + [ref_dev, diff, row_out]:
        a.free()
    dev.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_neutral_and_equal(dtype):
    nx, ny, g = 130, 9, 4
    params, arrays, host = _block(nx, ny, g, 4, dtype, seed=3)
    dev = params.device
    same = dev.from_host(np.stack([real(h, nx, ny, g) for h in host]).ravel())
    diff = dev.from_host(np.full(64, 0x5a5a5a5a5a5a5a5a, dtype=U64))
    reset(params, diff)
    assert records(params, diff, 8) == [(0, 0, 0, NONE, 0, NONE, 0, NONE)] * 8              # the neutral element
    assert compare_call(params, arrays, (0, 0, nx, ny), 0, nx, same, 0.0, 0.0, diff) == 0
    assert records(params, diff, 8) == [(nx * ny, 0, 0, NONE, 0, NONE, 0, NONE)] * 4 + [(0, 0, 0, NONE, 0, NONE, 0, NONE)] * 4
    for a in arrays + [same, diff]:
        a.free()
    dev.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_the_record_does_not_depend_on_the_split_the_alignment_or_the_ghost_width(dtype):
    nx, ny, g = 256, 70, 2
    rtol, atol = 4 * float(np.finfo(dtype).eps), 1e-13
    params, arrays, ours, ref = planted_pair(nx, ny, g, dtype, seed=99)
    dev = params.device
    diff, ref_dev = dev.empty(64, U64), dev.from_host(ref.ravel())
    reset(params, diff)
    assert compare_call(params, arrays, (0, 0, nx, ny), 0, nx, ref_dev, rtol, atol, diff) == 0
    params.wait()
    whole = diff.to_host().tobytes()
    reset(params, diff)
    assert compare_call(params, arrays, (0, 0, nx, ny), 0, nx, ref_dev, rtol, atol, diff) == 0
    params.wait()
    assert diff.to_host().tobytes() == whole                                              # two calls, the same bytes
    # a drawn partition into bands and column windows: single rows, single columns, odd starts and widths (element-wide path)
    rng = np.random.default_rng(5)
    row_cuts = sorted({0, 1, ny - 1, ny, *rng.integers(1, ny, 4).tolist()})
    col_cuts = sorted({0, 1, 2, nx - 1, nx, 128, *rng.integers(1, nx, 3).tolist()})
    reset(params, diff)
    n_windows, staged = 0, []
    for r0, r1 in zip(row_cuts, row_cuts[1:]):
        for c0, c1 in zip(col_cuts, col_cuts[1:]):
            dense = dev.from_host(np.ascontiguousarray(ref[:, r0:r1, c0:c1]).ravel())
            staged.append(dense)
            assert compare_call(params, arrays, (c0, r0, c1 - c0, r1 - r0), r0 * nx + c0, nx, dense, rtol, atol, diff) == 0
            n_windows += 1
    params.wait()
    assert n_windows >= 30 and diff.to_host().tobytes() == whole
    # the same state held with another ghost width
    other, oarrays, ohost = _block(nx, ny, 5, 3, dtype, seed=1)
    for a, h, o in zip(oarrays, ohost, ours):
        real(h, nx, ny, 5)[:] = o
        a.copy_from_host(h)
    odiff, oref = other.device.empty(64, U64), other.device.from_host(ref.ravel())
    reset(other, odiff)
    assert compare_call(other, oarrays, (0, 0, nx, ny), 0, nx, oref, rtol, atol, odiff) == 0
    other.wait()
    assert odiff.to_host().tobytes() == whole
    for a in arrays + staged + [diff, ref_dev]:
        a.free()
    for a in oarrays + [odiff, oref]:
        a.free()
    dev.close()
    other.device.close()


def test_ghost_cells_and_the_surroundings_of_the_dense_buffer_are_never_touched():
    nx, ny, g, pad = 37, 19, 3, 64
    params, arrays, ours, ref = planted_pair(nx, ny, g, "float64", seed=11)
    dev = params.device
    diff = dev.empty(64, U64)
    clean = dev.from_host(ref.ravel())
    reset(params, diff)
    assert compare_call(params, arrays, (0, 0, nx, ny), 0, nx, clean, 1e-10, 0.0, diff) == 0
    want = records(params, diff, 3)
    # NaN in every ghost cell of our vectors, a marker around the dense buffer
    poisoned = []
    for o in ours:
        full = np.full((ny + 2 * g, nx + 2 * g), np.nan)
        full[g:g + ny, g:g + nx] = o
        poisoned.append(full.ravel())
    for a, h in zip(arrays, poisoned):
        a.copy_from_host(h)
    framed = np.concatenate([np.full(pad, 7.5), ref.ravel(), np.full(pad, 7.5)])
    frame = dev.from_host(framed)
    reset(params, diff)
    assert compare_call(params, arrays, (0, 0, nx, ny), 0, nx, frame.ptr + pad * 8, 1e-10, 0.0, diff) == 0
    assert records(params, diff, 3) == want
    assert frame.to_host().tobytes() == framed.tobytes()
    for a, h in zip(arrays, poisoned):
        assert a.to_host().tobytes() == h.tobytes()
    for a in arrays + [diff, clean, frame]:
        a.free()
    dev.close()


def test_invalid_arguments_are_refused_and_leave_the_record_untouched():
    params, arrays, _ = _block(20, 10, 4, 8, "float64", seed=1)
    dev = params.device
    ref, diff = dev.zeros(9 * 200, "float64"), dev.from_host(np.arange(64, dtype=U64) + 1000)
    before = diff.to_host().tobytes()
    ok = ((0, 0, 20, 10), 0, 20, ref, 0.0, 0.0, diff)
    for win in ((1, 0, 20, 10), (0, 1, 20, 10), (-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 21, 1), (0, 0, 1, 11), (20, 0, 1, 1), (0, 0, 0, 5)):
        assert compare_call(params, arrays, win, *ok[1:]) == 1, win
    assert compare_call(params, arrays + arrays[:1], *ok, nvars=9) == 1
    assert compare_call(params, arrays, *ok, nvars=0) == 1
    assert compare_call(params, arrays, ok[0], 0, 20, None, 0.0, 0.0, diff) == 1
    assert compare_call(params, arrays, ok[0], 0, 20, ref, 0.0, 0.0, None) == 1
    for rtol, atol in ((-1e-300, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("nan"))):
        assert compare_call(params, arrays, ok[0], 0, 20, ref, rtol, atol, diff) == 1, (rtol, atol)
    assert compare_call(params, arrays, *ok, ctx=False) == 1
    assert compare_call(params, arrays, ok[0], 0, 19, ref, 0.0, 0.0, diff) == 1                 # a row longer than the domain's
    L = dev._L
    assert L.armon_hip_state_diff_reset(dev.ctx, 0, C.c_void_p(diff.ptr)) == 1 and L.armon_hip_state_diff_reset(dev.ctx, 9, C.c_void_p(diff.ptr)) == 1
    assert L.armon_hip_state_diff_reset(dev.ctx, 4, None) == 1
    params.wait()
    assert diff.to_host().tobytes() == before
    assert compare_call(params, arrays, *ok) == 0                                              # and the valid call still works
    params.wait()
    for a in arrays + [ref, diff]:
        a.free()
    dev.close()


# ---- file and grid ---------------------------------------------------------------------------------------------------------
SOD = dict(N=(96, 40), test="Sod", maxcycle=5, exact_arithmetic=True, silent=5)


def run(**kw):
    import armon_amd
    kw.setdefault("silent", 5)
    return armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **kw))


def change_cells(grid, name, cells, factor=1.5):
    """Change the real cells ``[(ix, iy)]`` (0-based) of one plane through state_unpack, one 1 x 1 window each → their old values."""
    p, dev = grid.params, grid.params.device
    host = grid.real_view(grid.data[name].to_host())
    digest, old = dev.zeros(8, U64), []
    for ix, iy in cells:
        old.append(host[iy, ix])
        one = dev.from_host(np.array([host[iy, ix] * factor + 0.25], dtype=p.data_type))
        ptrs = (C.c_void_p * 1)(grid.data[name].ptr)
        assert p.fn("state_unpack")(dev.ctx, grid.size.size[0], grid.size.ghosts, p.N[0], p.N[1], 1, ptrs, ix, iy, 1, 1,
                                    iy * p.N[0] + ix, p.N[0], C.c_void_p(one.ptr), C.c_void_p(digest.ptr)) == 0
        p.wait()
        one.free()
    digest.free()
    return old


def test_a_block_against_a_file_and_a_changed_cell(tmp_path):
    import armon_amd
    from armon_amd.compare import diff_reference
    stats = run(**SOD)
    grid = stats.data
    path = str(tmp_path / "a.ckpt")
    grid.save_state(path)
    clean = grid.compare_state(path, band_rows=7)
    assert not clean.different and list(clean.vars) == list(STATE)
    for f in STATE:
        assert clean[f].raw == (96 * 40, 0, 0, NONE, 0, NONE, 0, NONE) and clean[f].cells == []
    before = grid.real_view(grid.data["u"].to_host()).copy()
    (old,) = change_cells(grid, "u", [(50, 17)])
    after = grid.real_view(grid.data["u"].to_host())
    d = grid.compare_state(path, rtol=0.0, band_rows=7)
    assert d.different and [f for f in STATE if d[f].n_out] == ["u"]
    u = d["u"]
    assert u.raw == diff_reference(after, before, 0.0, 0.0)
    assert (u.n_out, u.n_bits, u.first_out, u.max_abs_at, u.max_rel_at) == (1, 1, (51, 18), (51, 18), (51, 18))
    assert u.max_abs == abs(old * 1.5 + 0.25 - old)
    assert u.cells == [(17 * 96 + 50, float(old), float(old * 1.5 + 0.25))]
    assert "1 differences found in u" in d.report("test") and "( 51, 18)" in d.report("test")
    assert grid.compare_state(path, rtol=0.0, limit=0)["u"].cells == []
    # a file with another N: a configuration error that names the field
    other = run(**{**SOD, "N": (40, 96)})
    with pytest.raises(armon_amd.SolverException) as e:
        other.data.compare_state(path)
    assert e.value.category == "config" and "N" in e.value.msg
    with pytest.raises(armon_amd.SolverException) as e:
        run(**{**SOD, "data_type": "float32"}).data.compare_state(path)
    assert e.value.category == "config" and "data_type" in e.value.msg


def test_tile_groups_return_the_single_blocks_result(tmp_path):
    from armon_amd.multi_tile import TileGroup
    block = run(**SOD).data
    path = str(tmp_path / "a.ckpt")
    block.save_state(path)
    cells = [(95, 3), (0, 4), (47, 4), (48, 20), (1, 20)]                      # five cells over three rows, on both sides of every cut
    groups = []
    try:
        for P in ((2, 2), (3, 1)):
            g = TileGroup(P, **SOD)
            g.run()
            groups.append(g)
            assert not g.compare_state(path, band_rows=7).different and not g.compare_state(block).different
            assert not block.compare_state(g).different
        # plant the same five cells in the block and in every tile group, through each tile's own state_unpack
        block_ref = run(**SOD).data
        change_cells(block, "u", cells)
        for g in groups:
            for p, t in zip(g.params, g.grids):
                ox, oy = p.N_origin[0] - 1, p.N_origin[1] - 1
                mine = [(ix - ox, iy - oy) for ix, iy in cells if ox <= ix < ox + p.N[0] and oy <= iy < oy + p.N[1]]
                change_cells(t, "u", mine)
        want_file = block.compare_state(path, rtol=0.0, band_rows=7)
        want_grid = block.compare_state(block_ref, rtol=0.0)
        assert want_file == want_grid and want_file["u"].n_out == 5
        assert [c[0] for c in want_file["u"].cells] == sorted(iy * 96 + ix for ix, iy in cells)
        three = block.compare_state(path, rtol=0.0, limit=3)
        assert [c[0] for c in three["u"].cells] == sorted(iy * 96 + ix for ix, iy in cells)[:3] and three["u"].raw == want_file["u"].raw
        for g in groups:
            assert g.compare_state(path, rtol=0.0, band_rows=7) == want_file, g.P
            assert g.compare_state(block_ref, rtol=0.0, band_rows=5) == want_file, g.P
            assert g.compare_state(path, rtol=0.0, limit=3) == three, g.P
            swapped = block_ref.compare_state(g, rtol=0.0)                 # a block against a group: d and m are symmetric,
            assert [swapped[f].raw for f in STATE] == [want_file[f].raw for f in STATE], g.P        # so the records are equal
            assert [c[0] for c in swapped["u"].cells] == [c[0] for c in want_file["u"].cells]
            assert [(c[2], c[1]) for c in swapped["u"].cells] == [(c[1], c[2]) for c in want_file["u"].cells]   # ref and ours swap
        assert groups[0].compare_state(groups[1], rtol=0.0)["u"].n_bits == 0                           # the same planted state
    finally:
        for g in groups:
            g.close()


def test_the_listing_fetches_a_bounded_number_of_rows_when_most_cells_differ(tmp_path):
    """Every cell of ``u`` and ``rho`` differs (the planes are overwritten with drawn values through state_unpack): the listing
    is the ``limit`` smallest indices, and it costs the rows that hold them, not the rows that differ."""
    from armon_amd import checkpoint
    from armon_amd.compare import cell_rule
    from armon_amd.multi_tile import TileGroup
    block, other = run(**SOD).data, run(**SOD).data
    path = str(tmp_path / "a.ckpt")
    other.save_state(path)
    p, dev = block.params, block.params.device
    drawn = np.random.default_rng(11).normal(size=(2, 40, 96))
    dense, digest = dev.from_host(drawn.reshape(-1)), dev.zeros(8, U64)
    checkpoint._move(p, block, ("rho", "u"), (0, 0, 96, 40), dense, digest, unpack=True)
    p.wait()
    dense.free()
    digest.free()
    before = other.real_view(other.data["u"].to_host())
    _, out, _, _ = cell_rule(drawn[1], before, 0.0, 0.0)
    assert out.sum() > 0.99 * 96 * 40
    where = np.flatnonzero(out.reshape(-1))
    group = TileGroup((2, 2), **SOD)
    try:
        group.run()
        for limit, rows in ((3, 1), (100, 2)):
            want = [(int(g), float(before.reshape(-1)[g]), float(drawn[1].reshape(-1)[g])) for g in where[:limit]]
            for ref, kw, pieces in ((path, dict(band_rows=7), 1), (other, dict(band_rows=7), 1), (group, dict(band_rows=5), 2)):
                d = block.compare_state(ref, rtol=0.0, limit=limit, **kw)
                assert d["u"].n_out == out.sum() and d["u"].cells == want, (limit, pieces)
                assert d["v"].n_out == 0 and d["v"].cells == []
                assert d.rows_fetched <= 2 * rows * pieces, (d.rows_fetched, limit, pieces)         # two planes differ
            d = group.compare_state(block, rtol=0.0, limit=limit, band_rows=5)     # the tiles of a group against the block
            assert [c[0] for c in d["u"].cells] == [int(g) for g in where[:limit]] and d.rows_fetched <= 2 * rows * 2
    finally:
        group.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
RUN = dict(N=(64, 48), test="Sod_circ", maxcycle=12, silent=5)


@pytest.fixture(scope="module")
def reference_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("reference")
    stats = run(exact_arithmetic=True, checkpoint_step=4, output_dir=str(d), **RUN)
    assert sorted(os.listdir(d)) == [f"checkpoint_{c:06d}.ckpt" for c in (4, 8, 12)]
    return str(d), stats


def assert_three_clean(stats, bits=True):
    assert stats.cycles == 12 and [c for c, _ in stats.state_diffs] == [4, 8, 12]
    for _, d in stats.state_diffs:
        assert not d.different and list(d.vars) == list(STATE)
        assert all(d[f].n_cells == 64 * 48 and d[f].n_out == 0 and (not bits or d[f].n_bits == 0) for f in STATE)


@pytest.mark.parametrize("variant", ["same", "staged", "nghost5"])
def test_a_run_compared_with_the_checkpoints_of_a_reference_run(reference_run, variant):
    d, _ = reference_run
    kw = {"same": dict(exact_arithmetic=True), "staged": dict(use_fused_sweep=False), "nghost5": dict(exact_arithmetic=True, nghost=5)}[variant]
    stats = run(compare_step=4, compare_at_end=True, compare_dir=d, **kw, **RUN)
    assert_three_clean(stats)
    assert stats.data.params.use_fused_sweep == (variant != "staged")


def test_a_tile_group_compared_with_the_checkpoints_of_a_block(reference_run):
    from armon_amd.multi_tile import TileGroup
    d, _ = reference_run
    group = TileGroup((2, 2), exact_arithmetic=True, compare_step=4, compare_at_end=True, compare_dir=d, **RUN)
    try:
        assert_three_clean(group.run())
    finally:
        group.close()


def test_the_tuned_run_is_within_its_stated_bar_and_not_bit_equal(reference_run):
    """tuned arithmetic within 1e-11 x max|field| of exact, per plane, the maxima taken from the reference file.
    The clock: rtol = 0 asks for the file's time bit for bit, and the tuned run's is one unit in the last place off at cycle 4
    (0.039790451281985668 against 0.039790451281985675, measured) — DESIGN §2 holds every tuned step to |dt - dt_ref| <= 1e-12
    dt_ref, the time is the sum of the steps, so |t - t_ref| <= 1e-12 t_ref; the smallest of these bounds (the first file's) is
    handed over as comparison_time_atol. The planes keep rtol = 0 and their own bar."""
    from armon_amd import checkpoint
    d, _ = reference_run
    path = os.path.join(d, "checkpoint_000012.ckpt")
    header = checkpoint.read_header(path)
    planes = np.fromfile(path, dtype=np.float64, offset=checkpoint.DATA_OFFSET).reshape(len(header["planes"]), 48, 64)
    atol = {f: 1e-11 * float(np.abs(planes[k]).max()) for k, f in enumerate(header["planes"])}
    first = checkpoint.read_header(os.path.join(d, "checkpoint_000004.ckpt"))
    stats = run(compare_step=4, compare_at_end=True, compare_dir=d, comparison_tolerance=0.0, comparison_atol=atol,
                comparison_time_atol=1e-12 * checkpoint.unhex(first["time"]), **RUN)
    for c, diff in stats.state_diffs:
        print(c, {f: (diff[f].n_bits, diff[f].n_out, diff[f].max_abs, atol[f]) for f in STATE})
    assert_three_clean(stats, bits=False)
    assert sum(diff[f].n_bits for _, diff in stats.state_diffs for f in STATE) > 0


def test_another_limiter_stops_the_run_at_the_first_comparison(reference_run, capsys):
    d, _ = reference_run
    stats = run(exact_arithmetic=True, riemann_limiter="superbee", compare_step=4, compare_at_end=True, compare_dir=d, **RUN)
    assert stats.cycles == 4 and [c for c, _ in stats.state_diffs] == [4]
    diff = stats.state_diffs[0][1]
    assert diff.different and any(diff[f].cells for f in STATE)
    out = capsys.readouterr().out
    assert "At cycle 4 against" in out and "differences found in" in out


def test_a_missing_file_or_another_cycle_is_an_io_error(reference_run, tmp_path):
    import armon_amd
    d, _ = reference_run
    with pytest.raises(armon_amd.SolverException) as e:
        run(exact_arithmetic=True, compare_step=3, compare_dir=d, **RUN)               # no file of cycle 3
    assert e.value.category == "io" and "checkpoint_000003.ckpt" in e.value.msg
    shutil.copy(os.path.join(d, "checkpoint_000008.ckpt"), tmp_path / "checkpoint_000004.ckpt")
    with pytest.raises(armon_amd.SolverException) as e:
        run(exact_arithmetic=True, compare_step=4, compare_dir=str(tmp_path), **RUN)   # the file of cycle 4 holds cycle 8
    assert e.value.category == "io" and "checkpoint_000004.ckpt" in e.value.msg


def test_the_defaults_change_nothing(reference_run):
    _, ref = reference_run
    a = run(exact_arithmetic=True, **RUN)
    b = run(exact_arithmetic=True, compare_step=0, compare_dir=None, compare_at_end=False, comparison_atol=0.0, **RUN)
    assert a.state_diffs == [] and b.state_diffs == []
    assert a.data.state_digest() == b.data.state_digest() == ref.data.state_digest()
    assert (a.cycles, a.final_time, a.last_dt) == (b.cycles, b.final_time, b.last_dt)
