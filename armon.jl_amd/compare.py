"""State comparison on the device (csrc/state_compare.hip): what separates the state of a run from a checkpoint, or from the
state of another run, reduced where the state lives to one 64-byte record per variable. No reference counterpart: the
reference compares text files on the host (ref src/io.jl:113-227; ``io.compare_host`` keeps that path as it is). A packed checkpoint (checkpoint.py, file version 2) is read through the
reader ``load_state`` uses, saved band by saved band, and gives the records of the unpacked file of the same state.

PER CELL, ``a`` = our value, ``b`` = the reference's, all arithmetic in the data type:

    same = (a == b) or both are NaN:  d = 0, relative difference 0      (equal infinities included)
    otherwise  d = |a - b|,  m = max(|a|, |b|),  relative difference d / m;  a NaN in either becomes the canonical quiet NaN
    within tolerance = same, or both finite and d <= max(atol, rtol m)

— Julia's ``isapprox`` as the reference's tests use it (ref test/reference_data/reference_functions.jl:54-57), two NaNs counted
as equal. ``n_bits`` counts the cells whose bit patterns differ (-0.0 against +0.0 does; it is within tolerance). MERGE: counts
add, ``first_out`` is a minimum, a (value, position) pair takes the larger bit pattern and on equal patterns the smaller
position; the position of a value of 0 is "none". Associative and commutative, so a record depends on the two states and
the tolerance only: not on the bands, the ghost width or the decomposition, and a tile group's record is the merge of its
tiles'. ``cell_rule`` / ``diff_reference`` below restate the rule in numpy; the listing uses them, and so do the tests.

A comparison streams the reference through the staging buffers of ``checkpoint._Pipeline`` (a file: band by band, host and
staging memory 2 x band) or packs the other grid's window next to ours (another grid: nothing touches the host), merges every
band into the record on the device without synchronising, and reads back ``nvars x 64`` bytes. Only when cells are out of
tolerance, and a listing was asked for, bands are looked at a second time, and only those that can still hold a smaller
global index than the cells held: a count per row (``row_out``) says which rows to fetch, those rows of both sides are fetched
in ascending order until ``limit`` cells per variable are held, and the cells are picked on the host with the same rule. The
listing costs at most ``limit`` rows per variable and piece, whether one cell differs or every one.
"""
import ctypes as C
import os

import numpy as np

from . import checkpoint
from ._lib import check, solver_error

NONE = (1 << 64) - 1
RAW_FIELDS = ("n_cells", "n_bits", "n_out", "first_out", "max_abs", "max_abs_at", "max_rel", "max_rel_at")
NEUTRAL = (0, 0, 0, NONE, 0, NONE, 0, NONE)


# ---- the rule, in numpy (the listing's cell picker and the tests' oracle) --------------------------------------------------
def _uint(dtype):
    return np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32


def cell_rule(ours, ref, rtol, atol):
    """→ (bits, out, d_bits, rel_bits): per cell whether the bit patterns differ, whether the cell is out of tolerance, and the
    bit patterns (uint64) of the absolute and relative difference as they enter the maxima."""
    a, b = np.asarray(ours), np.asarray(ref)
    T, U = a.dtype.type, _uint(a.dtype)
    assert a.dtype == b.dtype and a.dtype in (np.float64, np.float32) and a.shape == b.shape
    with np.errstate(all="ignore"):
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        d = np.abs(a - b)
        m = np.maximum(np.abs(a), np.abs(b))
        rel = d / m
        tol = np.maximum(T(atol), T(rtol) * m)
        within = same | (np.isfinite(a) & np.isfinite(b) & (d <= tol))
    quiet = U(0x7ff8000000000000 if U is np.uint64 else 0x7fc00000)

    def pattern(v):
        p = np.ascontiguousarray(v).view(U).copy()
        p[np.isnan(v)] = quiet
        p[same] = 0
        return p.astype(np.uint64)
    bits = np.ascontiguousarray(a).view(U) != np.ascontiguousarray(b).view(U)
    return bits, ~within, pattern(d), pattern(rel)


def diff_reference(ours, ref, rtol, atol, global_nx=None, origin=(0, 0)):
    """The record of the 2-D arrays ``ours`` against ``ref``, their first cell at global ``origin = (gx, gy)`` of a domain whose
    rows are ``global_nx`` long → tuple of the eight integers of ``armon_state_diff``."""
    ny, nx = np.shape(ours)
    global_nx = nx if global_nx is None else int(global_nx)
    bits, out, d, rel = cell_rule(ours, ref, rtol, atol)
    g = ((np.arange(ny, dtype=np.uint64)[:, None] + np.uint64(origin[1])) * np.uint64(global_nx)
         + np.arange(nx, dtype=np.uint64)[None, :] + np.uint64(origin[0]))

    def pair(p):
        top = int(p.max())
        return (top, int(g[p == top].min())) if top else (0, NONE)
    return (nx * ny, int(bits.sum()), int(out.sum()), int(g[out].min()) if out.any() else NONE) + pair(d) + pair(rel)


def merge_raw(x, y):
    """The merge of two records given as tuples of eight integers."""
    def pair(v1, a1, v2, a2):
        return (v2, a2) if (v2 > v1 or (v2 == v1 and a2 < a1)) else (v1, a1)
    return ((x[0] + y[0]) & NONE, (x[1] + y[1]) & NONE, (x[2] + y[2]) & NONE, min(x[3], y[3])) \
        + pair(x[4], x[5], y[4], y[5]) + pair(x[6], x[7], y[6], y[7])


# ---- the result ------------------------------------------------------------------------------------------------------------
class VarDiff:
    """One variable's record: ``raw`` (the eight integers), and decoded — the maxima as floats, the positions as 1-based
    ``(ix, iy)`` like the reference prints them (``None`` = no such cell) — plus ``cells``: the listed out-of-tolerance cells,
    ``(g, ref, ours)`` by ascending global index."""

    def __init__(self, raw, dtype, global_nx, cells=()):
        self.raw = tuple(int(v) for v in raw)
        self.dtype, self.global_nx = np.dtype(dtype), int(global_nx)
        self.cells = list(cells)

    n_cells = property(lambda self: self.raw[0])
    n_bits = property(lambda self: self.raw[1])
    n_out = property(lambda self: self.raw[2])

    def position(self, g):
        return None if g == NONE else (g % self.global_nx + 1, g // self.global_nx + 1)

    def value(self, pattern):
        return float(np.array([pattern], dtype=_uint(self.dtype)).view(self.dtype)[0])

    first_out = property(lambda self: self.position(self.raw[3]))
    max_abs = property(lambda self: self.value(self.raw[4]))
    max_abs_at = property(lambda self: self.position(self.raw[5]))
    max_rel = property(lambda self: self.value(self.raw[6]))
    max_rel_at = property(lambda self: self.position(self.raw[7]))

    def merge(self, other, limit=None):
        assert (self.dtype, self.global_nx) == (other.dtype, other.global_nx)
        cells = sorted({c[0]: c for c in self.cells + other.cells}.values(), key=lambda c: c[0])
        return VarDiff(merge_raw(self.raw, other.raw), self.dtype, self.global_nx, cells if limit is None else cells[:limit])

    def __eq__(self, other):
        def key(cells):      # NaN-proof: values by bit pattern
            return [(g, np.array([r, o], dtype=self.dtype).tobytes()) for g, r, o in cells]
        return isinstance(other, VarDiff) and (self.raw, self.dtype, self.global_nx) == (other.raw, other.dtype, other.global_nx) \
            and key(self.cells) == key(other.cells)

    def __repr__(self):
        return f"VarDiff({dict(zip(RAW_FIELDS, self.raw))}, cells={self.cells})"


class StateDiff:
    """``vars``: name → ``VarDiff``; ``limit``: how many cells per variable a listing keeps (the smallest global indices);
    ``time``: ``(ref, ours)`` when the clocks were compared and differ beyond the tolerance, else ``None``."""

    def __init__(self, vars, limit=20, time=None):
        self.vars, self.limit, self.time = dict(vars), int(limit), time
        self.rows_fetched = 0               # rows the listing fetched from the device (its cost; not part of the result)

    def __getitem__(self, name):
        return self.vars[name]

    @property
    def different(self):
        return self.time is not None or any(v.n_out > 0 for v in self.vars.values())

    def merge(self, other):
        assert list(self.vars) == list(other.vars)
        return StateDiff({k: v.merge(other.vars[k], min(self.limit, other.limit)) for k, v in self.vars.items()},
                         min(self.limit, other.limit), self.time if self.time is not None else other.time)

    def __eq__(self, other):
        return isinstance(other, StateDiff) and self.vars == other.vars and self.time == other.time

    def report(self, label):
        """The text of ``io.compare_host`` — "At label:", "n differences found in v", up to ``limit`` lines
        ``(ix, iy): ref ≢ ours (diff)`` — then the maxima and where they are → str."""
        lines = [f"At {label}:"]
        if self.time is not None:
            ref, ours = self.time
            lines.append(f"Time difference: ref t = {ref:.18f}, t = {ours:.18f}, diff = {ref - ours:.18f}")
        for name, v in self.vars.items():
            if v.n_out:
                lines.append(f"  {v.n_out} differences found in {name}")
                for g, ref, ours in v.cells[:self.limit]:
                    ix, iy = v.position(g)
                    with np.errstate(all="ignore"):
                        delta = v.dtype.type(ref) - v.dtype.type(ours)
                    lines.append(f"   - ({ix:3d},{iy:3d}): {ref:12.5g} ≢ {ours:12.5g} ({delta:12.5g})")
            if v.raw[4]:
                lines.append(f"  max |Δ{name}| = {v.max_abs:.5g} at {v.max_abs_at}, max |Δ{name}| / max(|ref|, |{name}|) = "
                             f"{v.max_rel:.5g} at {v.max_rel_at}, {v.n_bits} of {v.n_cells} cells differ in their bits")
        return "\n".join(lines)

    def __repr__(self):
        return f"StateDiff({self.vars}, time={self.time})"


# ---- device side -----------------------------------------------------------------------------------------------------------
def _atol_groups(names, atol):
    """``atol`` = one number for every variable, or a dict name → number (a bar per plane): the kernel takes one tolerance
    per call, and a call reads only its own planes → [(first variable, count, atol)]."""
    if isinstance(atol, dict):
        missing = [f for f in names if f not in atol]
        if missing:
            solver_error("config", f"atol has no entry for {missing}")
        groups = []
        for k, f in enumerate(names):                       # neighbours with the same bar share a launch
            if groups and groups[-1][2] == float(atol[f]):
                groups[-1] = (groups[-1][0], groups[-1][1] + 1, groups[-1][2])
            else:
                groups.append((k, 1, float(atol[f])))
        return groups
    return [(0, len(names), float(atol))]


def _check_tolerance(rtol, atol):
    values = [rtol] + (list(atol.values()) if isinstance(atol, dict) else [atol])
    if not all(isinstance(v, (int, float, np.floating, np.integer)) and v >= 0 for v in values):       # (a NaN fails v >= 0)
        solver_error("config", f"tolerances must be numbers >= 0, got rtol = {rtol!r}, atol = {atol!r}")


def _compare_window(params, grid, names, window, ref_ptr, rtol, atol, diff, row_out=None):
    """armon_hip_state_compare of ``window = (col0, row0, wnx, wny)`` of the tile's real cells against the dense
    ``[len(names)][wny][wnx]`` at the device address ``ref_ptr``, merged into ``diff`` (and counted per row into ``row_out``)."""
    col0, row0, wnx, wny = window
    ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
    NX = params.global_grid[0]
    item = params.data_type.itemsize
    fn = params.fn("state_compare")
    for k0, n, tol in _atol_groups(names, atol):
        vars_ = (C.c_void_p * n)(*[grid.data[f].ptr for f in names[k0:k0 + n]])
        check(fn(params.device.ctx, grid.size.size[0], grid.size.ghosts, params.N[0], params.N[1], n, vars_, col0, row0, wnx, wny,
                 (oy + row0) * NX + ox + col0, NX, C.c_void_p(ref_ptr + k0 * wny * wnx * item), float(rtol), tol,
                 C.c_void_p(diff.ptr + 64 * k0), C.c_void_p(row_out.ptr + 4 * k0 * wny) if row_out is not None else None))


def _reset(params, diff, nvars):
    check(params.device._L.armon_hip_state_diff_reset(params.device.ctx, nvars, C.c_void_p(diff.ptr)))


def _records(params, diff, nvars):
    params.wait()
    return [tuple(int(v) for v in r) for r in diff.to_host().reshape(8, 8)[:nvars]]


def _d2h(dev, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    check(dev._L.armon_hip_memcpy(dev.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2))
    return out


def _g_range(params, window):
    """The smallest and the largest global index of ``window = (col0, row0, wnx, wny)`` of the tile's real cells."""
    col0, row0, wnx, wny = window
    NX = params.global_grid[0]
    g0 = (params.N_origin[1] - 1 + row0) * NX + params.N_origin[0] - 1 + col0
    return g0, g0 + (wny - 1) * NX + wnx - 1


class _Lister:
    """The listing of a comparison: per variable the ``limit`` smallest global indices among the out-of-tolerance cells seen so
    far, ``(g, ref, ours)`` ascending, trimmed after every row. A band or a row is looked at only while it can still hold a
    smaller index than the ones held: at most ``limit`` rows per variable and piece are ever fetched (``rows_fetched`` counts
    them), however many cells differ."""

    def __init__(self, names, rtol, atol, limit):
        self.names, self.rtol, self.limit = names, rtol, limit
        self.atol = {f: tol for k0, n, tol in _atol_groups(names, atol) for f in names[k0:k0 + n]}
        self.cells = {f: [] for f in names}
        self.rows_fetched = 0

    def tile(self, params, grid, records):
        """The next tile, whose records (of the first pass) say how many cells are to be found and from where on."""
        self.params, self.grid = params, grid
        self.left = {f: r[2] for f, r in zip(self.names, records)}          # out-of-tolerance cells of the tile not seen yet
        self.first = {f: r[3] for f, r in zip(self.names, records)}

    def _wants(self, f, g_first):
        held = self.cells[f]
        return len(held) < self.limit or g_first < held[-1][0]

    def wants(self, window):
        """Whether ``window`` of the tile can still add to the listing of any variable."""
        g_first, g_last = _g_range(self.params, window)
        return any(self.left[f] and self.first[f] <= g_last and self._wants(f, g_first) for f in self.names)

    def band(self, window, counts, ref_row):
        """``counts`` = the band's ``row_out`` as ``[nvars][wny]``; ``ref_row(k, r)`` → the reference's row ``r`` of variable
        ``k`` of the window. Rows are taken in ascending order, and only while they can hold a smaller index."""
        col0, row0, wnx, wny = window
        g, pitch = self.grid.size.ghosts, self.grid.size.size[0]
        for k, f in enumerate(self.names):
            self.left[f] -= int(counts[k].sum())
            for r in np.flatnonzero(counts[k]):
                g0, _ = _g_range(self.params, (col0, row0 + int(r), wnx, 1))
                if not self._wants(f, g0):
                    break
                ours = self.grid.gather((f,), (g + row0 + int(r)) * pitch + g + col0, 1, wnx)[f]
                ref = ref_row(k, int(r))
                self.rows_fetched += 1
                _, out, _, _ = cell_rule(ours, ref, self.rtol, self.atol[f])
                new = [(g0 + int(i), float(ref[i]), float(ours[i])) for i in np.flatnonzero(out)[:self.limit]]
                self.cells[f] = sorted(self.cells[f] + new, key=lambda c: c[0])[:self.limit]


def _read_band(fd, params, header, names, pipe, s, r0, rows):
    """The rows [r0, r0 + rows) of this tile's window of the file's planes ``names`` → the pinned buffer ``s``, and on to its
    staging buffer (asynchronously)."""
    nx, item = params.N[0], params.data_type.itemsize
    band = pipe.host[s].array.view(np.uint8)
    for q, f in enumerate(names):
        for off, n, at in checkpoint._file_runs(params, names, header["planes"].index(f), r0, rows):
            lo = (q * rows * nx + at) * item
            got = os.preadv(fd, [memoryview(band[lo:lo + n * item])], off)
            if got != n * item:
                solver_error("io", f"truncated checkpoint: {got} of {n * item} bytes at offset {off}")
    pipe.host[s].copy_to_device_async(pipe.stage[s], n=len(names) * rows * nx)


def _tile_against_packed(fd, path, header, packed, params, grid, names, rtol, atol):
    """A packed file: the saved bands that intersect this tile, decoded by the reader ``load_state`` uses
    (checkpoint.packed_pieces), each compared where it lands and merged on the device → the tile's records."""
    dev = params.device
    diff = dev.empty(64, np.uint64)
    try:
        _reset(params, diff, len(names))
        for window, dense in checkpoint.packed_pieces(fd, path, header, packed, params, names):
            _compare_window(params, grid, names, window, dense.ptr, rtol, atol, diff)
        return _records(params, diff, len(names))
    finally:
        params.wait()
        diff.free()


def _list_against_packed(fd, path, header, packed, params, grid, names, rtol, atol, lister):
    """The second pass over a packed file: only the saved bands that can still add to the listing are decoded again; the
    reference's rows come from the decoded band on the device."""
    dev, nvars, item = params.device, len(names), params.data_type.itemsize
    diff = row_out = None
    try:
        diff = dev.empty(64, np.uint64)
        for window, dense in checkpoint.packed_pieces(fd, path, header, packed, params, names, want=lister.wants):
            if not lister.wants(window):
                continue                                            # (the pieces before this one may have filled the listing)
            wnx, rows = window[2], window[3]
            if row_out is None or len(row_out) < nvars * rows:
                if row_out is not None:
                    params.wait()
                    row_out.free()
                row_out = dev.empty(nvars * rows, np.uint32)
            row_out.fill_bytes(0)
            _reset(params, diff, nvars)
            _compare_window(params, grid, names, window, dense.ptr, rtol, atol, diff, row_out)
            if any(r[2] for r in _records(params, diff, nvars)):
                counts = row_out.to_host()[:nvars * rows].reshape(nvars, rows)
                lister.band(window, counts,
                            lambda q, r: _d2h(dev, dense.ptr + ((q * rows + r) * wnx) * item, wnx, params.data_type))
    finally:
        params.wait()
        for a in (diff, row_out):
            if a is not None:
                a.free()


def _tile_against_file(fd, header, params, grid, names, rtol, atol, band_rows):
    """Stream this tile's window of the file's planes through the pipeline (checkpoint._load_tile's direction) into
    state_compare → the tile's records. The bands merge on the device; the host waits for a buffer, never for a result."""
    dev, nx = params.device, params.N[0]
    pipe = checkpoint._Pipeline(params, len(names), band_rows)
    diff = None
    try:
        diff = dev.empty(64, np.uint64)
        _reset(params, diff, len(names))
        for k, (r0, rows) in enumerate(pipe.bands):
            s = k & 1
            if k >= 2:
                dev.event_sync(checkpoint.BAND_EVENT_SLOT + s)       # band k - 2 has left this pair of buffers
            _read_band(fd, params, header, names, pipe, s, r0, rows)
            _compare_window(params, grid, names, (0, r0, nx, rows), pipe.stage[s].ptr, rtol, atol, diff)
            dev.event_record(checkpoint.BAND_EVENT_SLOT + s)
        return _records(params, diff, len(names))
    finally:
        if diff is not None:
            diff.free()
        pipe.free()


def _list_against_file(fd, header, params, grid, names, rtol, atol, band_rows, lister):
    """The second pass over a tile that has cells out of tolerance: only the bands that can still add to the listing are read
    again, one at a time, with the per-row counts; the lister fetches the rows it needs."""
    dev, nx = params.device, params.N[0]
    pipe = checkpoint._Pipeline(params, len(names), band_rows)
    diff = row_out = None
    try:
        diff = dev.empty(64, np.uint64)
        row_out = dev.empty(len(names) * pipe.band_rows, np.uint32)
        for r0, rows in pipe.bands:
            window = (0, r0, nx, rows)
            if not lister.wants(window):
                continue
            _read_band(fd, params, header, names, pipe, 0, r0, rows)
            row_out.fill_bytes(0)
            _reset(params, diff, len(names))
            _compare_window(params, grid, names, window, pipe.stage[0].ptr, rtol, atol, diff, row_out)
            if any(r[2] for r in _records(params, diff, len(names))):
                counts = row_out.to_host()[:len(names) * rows].reshape(len(names), rows)
                ref = pipe.host[0].array[:len(names) * rows * nx].reshape(len(names), rows, nx)
                lister.band(window, counts, lambda q, r: ref[q, r])
    finally:
        for a in (diff, row_out):
            if a is not None:
                a.free()
        pipe.free()


def _overlap(p, o):
    """The real cells the tiles ``p`` and ``o`` (parameter sets of two decompositions of one domain) share →
    (gx0, gy0, wnx, wny) in global 0-based cells, or None."""
    x0, y0 = max(p.N_origin[0], o.N_origin[0]) - 1, max(p.N_origin[1], o.N_origin[1]) - 1
    x1 = min(p.N_origin[0] + p.N[0], o.N_origin[0] + o.N[0]) - 1
    y1 = min(p.N_origin[1] + p.N[1], o.N_origin[1] + o.N[1]) - 1
    return (x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else None


def _pieces(params, others, nvars, band_rows):
    """Our tile cut at the boundaries of the other grid's tiles → per piece ``(op, og, wnx, rows_max, bands)``, ``bands`` =
    [(the band's window in their tile, the same cells' window in ours)]."""
    item = params.data_type.itemsize
    for op, og in others:
        cut = _overlap(params, op)
        if cut is None:
            continue
        gx0, gy0, wnx, wny = cut
        rows_max = band_rows if band_rows is not None else checkpoint.BAND_BYTES // max(nvars * wnx * item, 1)
        rows_max = int(min(max(int(rows_max), 1), wny))
        bands = []
        for b0 in range(0, wny, rows_max):
            rows = min(rows_max, wny - b0)
            bands.append(((gx0 - (op.N_origin[0] - 1), gy0 + b0 - (op.N_origin[1] - 1), wnx, rows),
                          (gx0 - (params.N_origin[0] - 1), gy0 + b0 - (params.N_origin[1] - 1), wnx, rows)))
        yield op, og, wnx, rows_max, bands


class _Packer:
    """The other side's window, packed dense (armon_hip_state_pack) where our compare kernel reads it. Same device: the pack
    runs on OUR stream from their vectors (they are at rest), so pack and compare of every band are ordered by the stream and
    one buffer serves with no host synchronisation. Another device: the pack runs on theirs and the band is copied over, with
    a host wait on either side of the copy."""

    def __init__(self, params, op, n):
        self.params, self.op = params, op
        dev, odev = params.device, op.device
        self.remote = odev.device_id != dev.device_id
        self.stage = self.mine = self.scratch = None
        try:
            self.stage = odev.empty(n, params.data_type)
            self.scratch = odev.zeros(8, np.uint64)                 # the pack's digest words: not used
            if self.remote:
                self.mine = dev.empty(n, params.data_type)
        except BaseException:
            self.free()
            raise

    def pack(self, og, names, window):
        """→ the device address of the dense ``[len(names)][wny][wnx]`` of ``window`` of their tile."""
        params, op = self.params, self.op
        if not self.remote:
            col0, row0, wnx, wny = window
            NX = op.global_grid[0]
            vars_ = (C.c_void_p * len(names))(*[og.data[f].ptr for f in names])
            check(params.fn("state_pack")(params.device.ctx, og.size.size[0], og.size.ghosts, op.N[0], op.N[1], len(names), vars_,
                                          col0, row0, wnx, wny, _g_range(op, window)[0], NX, C.c_void_p(self.stage.ptr),
                                          C.c_void_p(self.scratch.ptr)))
            return self.stage.ptr
        params.wait()                                               # our copy of the band before has been compared
        checkpoint._move(op, og, names, window, self.stage, self.scratch)
        op.wait()
        nbytes = len(names) * window[2] * window[3] * params.data_type.itemsize
        check(params.device._L.armon_hip_memcpy(params.device.ctx, C.c_void_p(self.mine.ptr), C.c_void_p(self.stage.ptr), nbytes, 3))
        params.wait()                                               # their buffer is free for the next pack
        return self.mine.ptr

    def free(self):
        self.params.wait()
        for a in (self.stage, self.mine, self.scratch):
            if a is not None:
                a.free()
        self.stage = self.mine = self.scratch = None


def _tile_against_tiles(params, grid, others, names, rtol, atol, band_rows):
    """Our tile against the tiles of another grid that cover it: the window is cut at their boundaries, each piece is packed
    from the other side's vectors band by band and compared with ours, every band merged on the device → the tile's records,
    the only thing that touches the host."""
    dev, nvars = params.device, len(names)
    diff, packers = dev.empty(64, np.uint64), []
    try:
        _reset(params, diff, nvars)
        for op, og, wnx, rows_max, bands in _pieces(params, others, nvars, band_rows):
            packers.append(_Packer(params, op, nvars * rows_max * wnx))
            for theirs, ours in bands:
                _compare_window(params, grid, names, ours, packers[-1].pack(og, names, theirs), rtol, atol, diff)
        return _records(params, diff, nvars)
    finally:
        for packer in packers:                                      # (after the records: freeing waits for the stream)
            packer.free()
        diff.free()


def _list_against_tiles(params, grid, others, names, rtol, atol, band_rows, lister):
    """The second pass of ``_tile_against_tiles``: the bands that can still add to the listing, with the per-row counts; the
    reference's rows come from the packed band on the device."""
    dev, nvars, item = params.device, len(names), params.data_type.itemsize
    diff = dev.empty(64, np.uint64)
    try:
        for op, og, wnx, rows_max, bands in _pieces(params, others, nvars, band_rows):
            if not any(lister.wants(ours) for _, ours in bands):
                continue
            packer = _Packer(params, op, nvars * rows_max * wnx)
            row_out = None
            try:
                row_out = dev.empty(nvars * rows_max, np.uint32)
                for theirs, ours in bands:
                    if not lister.wants(ours):
                        continue
                    rows = ours[3]
                    ref = packer.pack(og, names, theirs)
                    row_out.fill_bytes(0)
                    _reset(params, diff, nvars)
                    _compare_window(params, grid, names, ours, ref, rtol, atol, diff, row_out)
                    if any(r[2] for r in _records(params, diff, nvars)):
                        counts = row_out.to_host()[:nvars * rows].reshape(nvars, rows)
                        lister.band(ours, counts, lambda q, r: _d2h(dev, ref + ((q * rows + r) * wnx) * item, wnx, params.data_type))
            finally:
                if row_out is not None:
                    row_out.free()
                packer.free()
    finally:
        diff.free()


# ---- a whole comparison ----------------------------------------------------------------------------------------------------
def _tiles_of(obj):
    """``(params, grid)`` of every tile of a ``BlockGrid`` or a ``TileGroup``, at rest."""
    if hasattr(obj, "_tiles_at_rest"):
        return obj._tiles_at_rest()
    obj.params.wait()
    return [(obj.params, obj)]


def check_comparable(params, N, data_type, what):
    """A configuration error that names the field: only the global grid and the data type have to agree — every option that
    decides bits (scheme, arithmetic, path, ghost width, decomposition) may differ: that is what a comparison is for."""
    if list(N) != list(params.global_grid):
        solver_error("config", f"{what} has N = {list(N)!r}, this run has N = {list(params.global_grid)!r}")
    if np.dtype(data_type) != params.data_type:
        solver_error("config", f"{what} has data_type = {np.dtype(data_type).name!r}, this run has data_type = {params.data_type.name!r}")


def compare_state(tiles, ref, rtol=None, atol=0.0, names=None, limit=20, band_rows=None, header=None):
    """The state held by the ``(params, grid)`` of ``tiles`` (idle) against ``ref`` — the path of a checkpoint (``header``: its
    header when the caller has read it already), or a ``BlockGrid`` / ``TileGroup`` of the same global ``N`` and data type,
    whatever its ghost width and decomposition → ``StateDiff``. ``rtol=None``: the ``comparison_tolerance`` option; ``atol``: a
    number, or a dict name → number; ``names``: the planes to compare (default: ``checkpoint.plane_names`` of this run
    restricted to what both sides have); ``limit``: how many out-of-tolerance cells per variable are listed (0 = none: then
    nothing but the records is ever read back). The listing costs at most ``limit`` rows per variable and piece, however many
    cells differ. A file's digests are NOT verified here (``load_state`` does that); only its header is checked."""
    p0 = tiles[0][0]
    rtol = p0.comparison_tolerance if rtol is None else rtol
    _check_tolerance(rtol, atol)
    NX = p0.global_grid[0]
    fd = others = None
    if isinstance(ref, (str, os.PathLike)):
        ref = str(ref)
        header = checkpoint.read_header(ref) if header is None else header
        check_comparable(p0, header["N"], header["data_type"], f"the checkpoint {ref}")
        checkpoint.check_same_gravity(p0, header, f"the checkpoint {ref}")      # a state under another body force is another problem
        checkpoint.check_same_periodic(p0, header, f"the checkpoint {ref}")     # and so is one under other boundaries
        checkpoint.check_same_scalars(p0, header, f"the checkpoint {ref}")      # and the planes of other scalars are other fields
        checkpoint.check_same_diffusion(p0, header, f"the checkpoint {ref}")    # and a state under other diffusion coefficients
        checkpoint.check_same_transport(p0, header, f"the checkpoint {ref}")    # and planes carried by another transport rule
        theirs = tuple(header["planes"])
    else:
        header, others = None, _tiles_of(ref)
        check_comparable(p0, others[0][0].global_grid, others[0][0].data_type, "the other grid")
        checkpoint.check_same_gravity(p0, checkpoint.bit_options(others[0][0]), "the other grid")
        checkpoint.check_same_periodic(p0, checkpoint.bit_options(others[0][0]), "the other grid")
        checkpoint.check_same_scalars(p0, checkpoint.bit_options(others[0][0]), "the other grid")
        checkpoint.check_same_diffusion(p0, checkpoint.bit_options(others[0][0]), "the other grid")
        checkpoint.check_same_transport(p0, checkpoint.bit_options(others[0][0]), "the other grid")
        theirs = checkpoint.plane_names(others[0][0])
    if names is None:
        names = tuple(f for f in checkpoint.plane_names(p0) if f in theirs)
    names = tuple(names)
    if not 1 <= len(names) <= 8:
        solver_error("config", f"compare_state takes 1 to 8 planes, got {names!r}")
    if header is not None and any(f not in theirs for f in names):
        solver_error("config", f"the checkpoint {ref} holds the planes {theirs}, not all of {names}")
    lister = _Lister(names, rtol, atol, limit) if limit > 0 else None
    try:
        packed = None
        if header is not None:
            fd = os.open(ref, os.O_RDONLY)
            if checkpoint.is_packed(header):                        # chunks and an index: validated, then read band by saved band
                packed = checkpoint.read_index(ref, header, fd)
        total = [NEUTRAL] * len(names)
        for params, grid in tiles:
            if packed is not None:
                records = _tile_against_packed(fd, ref, header, packed, params, grid, names, rtol, atol)
            elif header is not None:
                records = _tile_against_file(fd, header, params, grid, names, rtol, atol, band_rows)
            else:
                records = _tile_against_tiles(params, grid, others, names, rtol, atol, band_rows)
            total = [merge_raw(t, r) for t, r in zip(total, records)]
            if lister is None or not any(r[2] for r in records):
                continue
            lister.tile(params, grid, records)
            if not lister.wants((0, 0, params.N[0], params.N[1])):
                continue                                            # every cell of this tile comes after the ones held
            if packed is not None:
                _list_against_packed(fd, ref, header, packed, params, grid, names, rtol, atol, lister)
            elif header is not None:
                _list_against_file(fd, header, params, grid, names, rtol, atol, band_rows, lister)
            else:
                _list_against_tiles(params, grid, others, names, rtol, atol, band_rows, lister)
    except OSError as e:
        solver_error("io", f"cannot read the checkpoint {ref}: {e}")
    finally:
        if fd is not None:
            os.close(fd)
    diff = StateDiff({f: VarDiff(t, p0.data_type, NX, lister.cells[f] if lister else ()) for f, t in zip(names, total)}, limit)
    diff.rows_fetched = lister.rows_fetched if lister else 0
    return diff


# ---- the run options (compare_step, compare_dir, compare_file, compare_at_end) ---------------------------------------------
def compare_path(params, cycle):
    return os.path.join(params.compare_dir, f"{params.compare_file}_{cycle:06d}.ckpt")


def compare_run(owner, params, gdt):
    """The state of the run ``owner`` (a ``BlockGrid`` or a ``TileGroup``) after ``gdt.cycle`` completed cycles against the
    file of that cycle; the file's time against the run's under the same ``rtol`` and the clock's own absolute tolerance
    ``comparison_time_atol`` (the planes' are not times). The result joins ``owner.state_diffs``; the first one that is
    different is printed → whether the run has to stop (ref @checkpoint, src/solver.jl:40-55)."""
    path = compare_path(params, gdt.cycle)
    header = checkpoint.read_header(path)
    if header["cycle"] != gdt.cycle:
        solver_error("io", f"the checkpoint {path} is at cycle {header['cycle']}, the run at cycle {gdt.cycle}")
    diff = compare_state(_tiles_of(owner), path, atol=params.comparison_atol, header=header)
    T = params.T
    with np.errstate(all="ignore"):
        t_ref, t = T(checkpoint.unhex(header["time"])), T(gdt.time)
        tol = max(T(params.comparison_time_atol), T(params.comparison_tolerance) * max(abs(t_ref), abs(t)))
        if not (t_ref == t or abs(t_ref - t) <= tol):
            diff.time = (float(t_ref), float(t))
    owner.state_diffs.append((gdt.cycle, diff))
    if diff.different:
        print(diff.report(f"cycle {gdt.cycle} against {path}"))
    return diff.different
