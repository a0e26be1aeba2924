"""Checkpoint and bit-exact restart, with a state digest computed on the device (csrc/checkpoint.hip). No reference
counterpart: the reference's only state files are text at ``output_precision`` (ref src/io.jl:2-27).

File, in this order: the magic ``ARMONCKP``, a u32 version, a u32 header length, a UTF-8 JSON header padded with spaces to
4096 bytes, then the dense GLOBAL planes ``[NY][NX]`` of real cells, little-endian, in the order rho, u, v, E — and ``c`` as a
fifth plane when the run is staged (its ``next_time_step`` reads the ``c`` the last EOS of the previous cycle left). Ghost
cells are not stored: both paths rebuild them before any read. A fused run with passive scalars appends one
plane ``s:<name>`` per scalar (8 planes at most) and lists the names under ``scalars`` in the header; without scalars the
file is byte for byte what it was.

The digest of plane k is the sum mod 2^64 over its cells of ``mix64(b + mix64(8 g + k + 1))`` — ``b`` the value's bit pattern
zero-extended to 64 bits, ``g = gy NX + gx`` its global 0-based index, ``mix64`` as in ``mix64`` below. It depends on the
values and their global positions only, so the tiles of a group add their digests up to the single block's.

Pipeline: a tile's window is cut into row bands; band k is packed (and digested) into one of two device staging buffers,
copied asynchronously into one of two pinned host buffers, and written at its file offset while band k + 1 is being packed.
Host and staging memory are 2 x band, never a whole field. The band height comes from a byte budget of 256 MB per buffer —
large enough that a band's kernel and copy (tens of ms) dwarf their launch cost, small enough to be pinned without a thought
next to a 16384² run (8.6 GB per plane) — or from ``band_rows``. Restore runs the same bands the other way.

PACKED FILES (``compress=True``, the ``checkpoint_compress`` option): file version 2 in the preamble — the header's keys as they
are (its own ``version`` key included) plus ``codec`` ("xorplane16"), ``index_offset`` and ``index_count``. From ``DATA_OFFSET``
on come CHUNKS, back to back, 8-byte aligned, in the order they were written: every band of every tile gives one chunk per
plane, encoded on the device with the lossless codec of csrc/plane_codec.hip (``plane_codec.py`` restates it), or raw (dense
``[wny][wnx]``) when the encoding is not smaller. At ``index_offset`` sit ``index_count`` records of eight little-endian u64 — plane, codec (0 raw, 1 xorplane16), global
col0, global row0, wnx, wny, file offset, bytes — and the file ends with them. The digests are those of the values, so they
are the same in both versions; ``expand`` turns a packed file into the version-1 file of the same state on the host. Loading
and comparing read a packed file through ``packed_pieces``: saved band by saved band, whatever the reader's decomposition.
"""
import ctypes as C
import json
import os
import struct

import numpy as np

from . import plane_codec
from ._lib import check, solver_error

MAGIC = b"ARMONCKP"
VERSION = 1                               # dense planes; what a save without compression writes
VERSION_PACKED = 2                        # chunks and an index
CODEC = "xorplane16"
CODEC_RAW, CODEC_XORPLANE = 0, 1
INDEX_RECORD = 64                         # eight little-endian u64
PACKED_KEYS = ("codec", "index_offset", "index_count")
HEADER_BYTES = 4096                       # the JSON header, padded
DATA_OFFSET = len(MAGIC) + 4 + 4 + HEADER_BYTES
BAND_BYTES = 256 << 20                    # per staging / pinned buffer
BAND_EVENT_SLOT = 1016                    # event-pool slots 1016, 1017: one per staging buffer
STATE_PLANES = ("rho", "u", "v", "E")
MASK = (1 << 64) - 1

# every option that decides bits: a restart must agree with the file on all of them
BIT_FIELDS = ("data_type", "N", "test", "domain_size", "origin", "periodic", "scheme", "riemann_limiter", "projection", "axis_splitting",
              "eos", "cfl", "cst_dt", "Dt", "use_fused_sweep", "exact_arithmetic")
# only in the header of a user-defined problem (problem.py; "test" is then "Problem:<name>"): gamma as a hexfloat and the
# sha256 of the problem's canonical description
PROBLEM_FIELDS = ("gamma", "problem_digest")
# only in the header of a run under a body force: two hexfloats, the (gx, gy) the device receives. A header
# without the key is that of a run without a force — every header written before the option existed, byte for byte
NO_GRAVITY = [float(0.).hex(), float(0.).hex()]


# ---- digest (host restatement: tests, and files checked without a device) ------------------------------------------------
def mix64(z):
    """``z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31`` on uint64 arrays."""
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xbf58476d1ce4e5b9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94d049bb133111eb)
        z ^= z >> np.uint64(31)
    return z


def digest_reference(plane, k, global_nx=None, origin=(0, 0)):
    """Digest of the 2-D array ``plane`` as variable ``k``, its first cell at global ``origin = (gx, gy)`` of a domain whose
    rows are ``global_nx`` long (default: the plane's own width) → int."""
    plane = np.ascontiguousarray(plane)
    ny, nx = plane.shape
    global_nx = nx if global_nx is None else int(global_nx)
    b = plane.view(np.uint64 if plane.dtype.itemsize == 8 else np.uint32).astype(np.uint64)
    gy, gx = np.meshgrid(np.arange(ny, dtype=np.uint64) + np.uint64(origin[1]),
                         np.arange(nx, dtype=np.uint64) + np.uint64(origin[0]), indexing="ij")
    with np.errstate(over="ignore"):
        g = gy * np.uint64(global_nx) + gx
        terms = mix64(b + mix64(np.uint64(8) * g + np.uint64(k + 1)))
        return int(terms.sum(dtype=np.uint64))


# ---- header --------------------------------------------------------------------------------------------------------------
def hexfloat(v):
    """A float as text that carries every bit (``float.hex``; ``inf`` and ``nan`` pass through it too)."""
    return float(v).hex()


def unhex(s):
    return float.fromhex(s)


def write_header(f, header, version=VERSION):
    """The preamble at offset 0 of the open binary file ``f``: magic, version, header length, padded JSON."""
    text = json.dumps(header, sort_keys=True).encode("utf-8")
    if len(text) > HEADER_BYTES:
        solver_error("io", f"checkpoint header of {len(text)} bytes does not fit in {HEADER_BYTES}")
    f.seek(0)
    f.write(MAGIC + struct.pack("<II", version, len(text)) + text + b" " * (HEADER_BYTES - len(text)))


def read_header(path):
    """→ the header of the checkpoint ``path``, after checking the magic, the version and the file's length."""
    try:
        with open(path, "rb") as f:
            pre = f.read(DATA_OFFSET)
            size = os.fstat(f.fileno()).st_size
    except OSError as e:
        solver_error("io", f"cannot read the checkpoint {path}: {e}")
    if len(pre) < 16 or pre[:8] != MAGIC:
        solver_error("io", f"{path} is not a checkpoint: bad magic {pre[:8]!r}")
    version, length = struct.unpack("<II", pre[8:16])
    if version not in (VERSION, VERSION_PACKED):
        solver_error("io", f"{path}: checkpoint version {version}, this build reads versions {VERSION} and {VERSION_PACKED}")
    if length > HEADER_BYTES or len(pre) < DATA_OFFSET:
        solver_error("io", f"{path}: truncated or damaged header")
    try:
        header = json.loads(pre[16:16 + length].decode("utf-8"))
    except ValueError as e:
        solver_error("io", f"{path}: unreadable header: {e}")
    _check_header(header, path)
    NX, NY = header["N"]
    if version == VERSION_PACKED:
        at, count = header.get("index_offset"), header.get("index_count")
        if header.get("codec") != CODEC or not all(isinstance(v, int) and not isinstance(v, bool) for v in (at, count)) \
                or at < DATA_OFFSET or at % 8 or count < 1:
            solver_error("io", f"{path}: damaged checkpoint header: codec = {header.get('codec')!r}, index_offset = {at!r}, "
                               f"index_count = {count!r}")
        want = at + INDEX_RECORD * count
    else:
        if any(k in header for k in PACKED_KEYS):
            solver_error("io", f"{path}: damaged checkpoint header: a version {VERSION} file with the keys of a packed one")
        want = DATA_OFFSET + len(header["planes"]) * NX * NY * np.dtype(header["data_type"]).itemsize
    if size != want:
        solver_error("io", f"{path}: truncated checkpoint: {size} bytes, {want} expected")
    return header


def is_packed(header):
    return "index_offset" in header


def _is_hexfloat(v):
    try:
        return isinstance(v, str) and (float.fromhex(v), True)[1]
    except ValueError:
        return False


def _check_header(header, path):
    """A header that parses but does not have the shape ``save`` writes is a damaged file: an I/O error, never a KeyError."""
    def bad(what):
        solver_error("io", f"{path}: damaged checkpoint header: {what}")
    if not isinstance(header, dict):
        bad("not a JSON object")
    N, planes, digests = header.get("N"), header.get("planes"), header.get("digests")
    if not (isinstance(N, list) and len(N) == 2 and all(isinstance(n, int) and not isinstance(n, bool) and n >= 1 for n in N)):
        bad(f"N = {N!r}")
    if header.get("data_type") not in ("float64", "float32"):
        bad(f"data_type = {header.get('data_type')!r}")
    if not (isinstance(planes, list) and 1 <= len(planes) <= 8 and all(isinstance(f, str) for f in planes)):
        bad(f"planes = {planes!r}")
    if not (isinstance(digests, dict) and all(isinstance(digests.get(f), str) for f in planes)):
        bad(f"digests = {digests!r}")
    cycle = header.get("cycle")
    if not (isinstance(cycle, int) and not isinstance(cycle, bool) and cycle >= 0):
        bad(f"cycle = {cycle!r}")
    for k in ("time", "current_dt", "next_cycle_dt"):
        if not _is_hexfloat(header.get(k)):
            bad(f"{k} = {header.get(k)!r}")
    if "pending_dt" not in header or not (header["pending_dt"] is None or _is_hexfloat(header["pending_dt"])):
        bad(f"pending_dt = {header.get('pending_dt')!r}")
    if "gravity" in header and not (isinstance(header["gravity"], list) and len(header["gravity"]) == 2
                                    and all(_is_hexfloat(v) for v in header["gravity"])):
        bad(f"gravity = {header['gravity']!r}")
    if "scalars" in header and not (isinstance(header["scalars"], list) and 1 <= len(header["scalars"]) <= 4
                                    and all(isinstance(v, str) and v and ":" not in v for v in header["scalars"])):
        bad(f"scalars = {header['scalars']!r}")
    if "diffusion" in header:
        d = header["diffusion"]
        if not (isinstance(d, dict) and _is_hexfloat(d.get("nu")) and _is_hexfloat(d.get("chi")) and isinstance(d.get("scalars"), dict)
                and all(isinstance(k, str) and _is_hexfloat(v) for k, v in d["scalars"].items())):
            bad(f"diffusion = {d!r}")
    if "scalar_transport" in header and not (header["scalar_transport"] == "bounded" and "scalars" in header):
        bad(f"scalar_transport = {header['scalar_transport']!r}")       # (the default rule is not written)
    if ("initial_mass" in header or "initial_energy" in header) and not (
            _is_hexfloat(header.get("initial_mass")) and _is_hexfloat(header.get("initial_energy"))):
        bad("initial_mass / initial_energy")


def bit_options(params):
    """What decides the bits of a run, as the header stores it (floats as hex text)."""
    fused = bool(params.use_fused_sweep)
    test = params.test
    options = {"data_type": params.data_type.name, "N": list(params.global_grid),
               "domain_size": [hexfloat(v) for v in params.domain_size], "origin": [hexfloat(v) for v in params.origin],
               "periodic": [bool(v) for v in params.periodic], "test": getattr(test, "header_name", test.name), "scheme": params.riemann_scheme, "riemann_limiter": params.riemann_limiter,
               "projection": params.projection_scheme, "axis_splitting": params.axis_splitting, "eos": test.eos,
               "cfl": hexfloat(params.cfl), "cst_dt": bool(params.cst_dt), "Dt": hexfloat(params.Dt),
               "use_fused_sweep": fused, "exact_arithmetic": bool(params.exact_arithmetic) if fused else None}
    if getattr(test, "is_problem", False):      # a user-defined problem (problem.py): the headers of the built-in cases are untouched
        options.update(gamma=hexfloat(test.gamma), problem_digest=test.digest)
    gravity = tuple(getattr(test, "gravity", (0., 0.)))
    if gravity != (0., 0.):                     # a run under a body force: the headers of every other run are untouched
        options.update(gravity=[hexfloat(g) for g in gravity])
    scalars = list(getattr(params, "scalar_names", ()))
    if scalars:                                 # a run with passive scalars: likewise
        options.update(scalars=scalars)
    if getattr(params, "diffusive", False):     # a run with physical diffusion: likewise
        from .problem import diffusion_description
        options.update(diffusion=diffusion_description(params.viscosity, params.heat_diffusivity, params.scalars))
    transport = getattr(params, "scalar_transport", "remap")
    if transport != "remap":                    # scalars carried by another rule than the default: likewise
        options.update(scalar_transport=transport)
    return options


def check_same_transport(params, header, what):
    """A configuration error when ``header`` (a missing key = ``"remap"``) and the run disagree on the rule the sweeps carry the
    passive scalars with: the planes of one rule are not the planes of the other."""
    theirs, mine = header.get("scalar_transport", "remap"), getattr(params, "scalar_transport", "remap")
    if theirs != mine:
        solver_error("config", f"{what} was written with scalar_transport = {theirs!r}, this run has scalar_transport = {mine!r}")


def check_same_diffusion(params, header, what):
    """A configuration error when ``header`` (a missing key = nothing diffuses) and the run disagree on the coefficients of
    the physical diffusion: a state under other coefficients is the state of another problem."""
    theirs, mine = header.get("diffusion"), bit_options(params).get("diffusion")
    if theirs != mine:
        solver_error("config", f"{what} was written with diffusion = {theirs!r}, this run has diffusion = {mine!r}")


def check_same_gravity(params, header, what):
    """A configuration error when ``header`` (a missing key = no force) and the run disagree on the body force."""
    theirs, mine = header.get("gravity", NO_GRAVITY), bit_options(params).get("gravity", NO_GRAVITY)
    if theirs != mine:
        solver_error("config", f"{what} was written with gravity = {theirs!r}, this run has gravity = {mine!r}")


def check_same_scalars(params, header, what):
    """A configuration error when ``header`` (a missing key = none) and the run disagree on the names of the passive scalars,
    in plane order."""
    theirs, mine = list(header.get("scalars", [])), list(getattr(params, "scalar_names", ()))
    if theirs != mine:
        solver_error("config", f"{what} was written with scalars = {theirs!r}, this run has scalars = {mine!r}")


def check_same_periodic(params, header, what):
    """A configuration error when ``header`` and the run disagree on the periodic axes: a state under other
    boundaries is the state of another problem."""
    theirs, mine = list(header.get("periodic", [False, False])), [bool(v) for v in params.periodic]
    if theirs != mine:
        solver_error("config", f"{what} was written with periodic = {theirs!r}, this run has periodic = {mine!r}")


def check_compatible(params, header, path):
    """A configuration error that names the first bit-deciding field on which the file and the run disagree, or a file that
    leaves nothing to run. ``nghost``, the decomposition, ``maxcycle``, ``maxtime`` and the output options are free."""
    mine = bit_options(params)
    check_same_gravity(params, header, f"the checkpoint {path}")      # (first: a problem's digest holds its force too)
    check_same_scalars(params, header, f"the checkpoint {path}")      # (and its scalars)
    check_same_diffusion(params, header, f"the checkpoint {path}")    # (and its diffusion coefficients)
    check_same_transport(params, header, f"the checkpoint {path}")    # (and the rule its scalars are carried with)
    for k in BIT_FIELDS + PROBLEM_FIELDS:
        if header.get(k) != mine.get(k):
            solver_error("config", f"the checkpoint {path} was written with {k} = {header.get(k)!r}, this run has "
                                   f"{k} = {mine.get(k)!r}")
    if header["cycle"] >= params.maxcycle or params.T(unhex(header["time"])) >= params.T(params.maxtime):
        solver_error("config", f"the checkpoint {path} is at cycle {header['cycle']}, time {unhex(header['time'])}: nothing left "
                               f"to run with maxcycle = {params.maxcycle}, maxtime = {params.maxtime}")


def checkpoint_path(params, cycle):
    return os.path.join(params.output_dir, f"{params.checkpoint_file}_{cycle:06d}.ckpt")


def plane_names(params):
    """The planes of a run's checkpoint: the state, then ``s:<name>`` per passive scalar (fused path; DESIGN.md §4.14: 8
    planes at most, hence 4 scalars), or ``c`` on the staged path."""
    if not params.use_fused_sweep:
        return STATE_PLANES + ("c",)
    return STATE_PLANES + tuple("s:" + name for name in getattr(params, "scalar_names", ()))


# ---- device side ---------------------------------------------------------------------------------------------------------
def _move(params, grid, names, window, dense, digest, unpack=False):
    """armon_hip_state_pack / _unpack of ``window = (col0, row0, wnx, wny)`` of the tile's real cells."""
    col0, row0, wnx, wny = window
    ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
    NX = params.global_grid[0]
    vars_ = (C.c_void_p * len(names))(*[grid.data[f].ptr for f in names])
    fn = params.fn("state_unpack" if unpack else "state_pack")
    check(fn(params.device.ctx, grid.size.size[0], grid.size.ghosts, params.N[0], params.N[1], len(names), vars_, col0, row0,
             wnx, wny, (oy + row0) * NX + ox + col0, NX, C.c_void_p(dense.ptr) if dense is not None else None,
             C.c_void_p(digest.ptr)))


def _bands(params, nvars, band_rows):
    nx, ny = params.N
    if band_rows is None:
        band_rows = BAND_BYTES // max(nvars * nx * params.data_type.itemsize, 1)
    band_rows = int(min(max(int(band_rows), 1), ny))
    return band_rows, [(r0, min(band_rows, ny - r0)) for r0 in range(0, ny, band_rows)]


def state_digest(tiles, names):
    """Per name of ``names`` the digest of the whole domain the ``(params, grid)`` of ``tiles`` cover → tuple of ints."""
    if not 1 <= len(names) <= 8:
        solver_error("config", f"state_digest takes 1 to 8 vectors, got {len(names)}")
    total = [0] * len(names)
    for params, grid in tiles:
        dev = params.device
        digest = dev.zeros(8, np.uint64)
        try:
            _move(params, grid, names, (0, 0, params.N[0], params.N[1]), None, digest)
            params.wait()
            d = digest.to_host()
        finally:
            digest.free()
        total = [(t + int(v)) & MASK for t, v in zip(total, d)]
    return tuple(total)


class _Pipeline:
    """Two staging buffers on the device, two pinned ones on the host and the digest words of one tile."""

    def __init__(self, params, nvars, band_rows):
        dev = params.device
        self.params, self.nvars = params, nvars
        self.band_rows, self.bands = _bands(params, nvars, band_rows)
        n = nvars * self.band_rows * params.N[0]
        self.stage, self.host, self.digest = [], [], None
        try:
            self.digest = dev.zeros(8, np.uint64)
            for _ in range(min(2, len(self.bands))):
                self.stage.append(dev.empty(n, params.data_type))
                self.host.append(dev.pinned(n, params.data_type))
        except BaseException:
            self.free()
            raise

    def digests(self):
        self.params.wait()
        return [int(v) for v in self.digest.to_host()[:self.nvars]]

    def free(self):
        self.params.wait()
        for a in self.stage + self.host + ([self.digest] if self.digest is not None else []):
            a.free()
        self.stage, self.host, self.digest = [], [], None


def _file_runs(params, header_planes, q, r0, rows):
    """Where the rows [r0, r0 + rows) of this tile's plane ``q`` sit in the file → list of (offset, elements, first element in
    the band's dense plane): one run when the tile spans the global rows, one per row otherwise."""
    nx = params.N[0]
    NX, NY = params.global_grid
    ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
    item = params.data_type.itemsize
    base = DATA_OFFSET + (q * NY + oy + r0) * NX * item
    if nx == NX:
        return [(base, rows * nx, 0)]
    return [(base + (r * NX + ox) * item, nx, r * nx) for r in range(rows)]


def _pwrite_all(fd, data, offset):
    """``os.pwrite`` until every byte is out (a write may be short: a signal, a quota)."""
    done = 0
    while done < len(data):
        n = os.pwrite(fd, data[done:], offset + done)
        if n <= 0:
            raise OSError(f"short write: {done} of {len(data)} bytes at offset {offset}")
        done += n


def _save_tile(fd, params, grid, names, band_rows):
    """Pack, copy and write the bands of one tile → its per-plane digests."""
    dev, nx = params.device, params.N[0]
    pipe = _Pipeline(params, len(names), band_rows)
    try:
        def write(k):
            r0, rows = pipe.bands[k]
            dev.event_sync(BAND_EVENT_SLOT + (k & 1))
            band = pipe.host[k & 1].array.view(np.uint8)
            item = params.data_type.itemsize
            for q in range(len(names)):
                for off, n, at in _file_runs(params, names, q, r0, rows):
                    lo = (q * rows * nx + at) * item
                    _pwrite_all(fd, memoryview(band[lo:lo + n * item]), off)

        for k, (r0, rows) in enumerate(pipe.bands):
            s = k & 1
            _move(params, grid, names, (0, r0, nx, rows), pipe.stage[s], pipe.digest)
            pipe.host[s].copy_from_device_async(pipe.stage[s], n=len(names) * rows * nx)
            dev.event_record(BAND_EVENT_SLOT + s)
            if k > 0:
                write(k - 1)                      # while band k is packed and copied
        write(len(pipe.bands) - 1)
        return pipe.digests()
    finally:
        pipe.free()


def _load_tile(fd, params, grid, names, band_rows):
    """Read, copy and unpack the bands of one tile → the per-plane digests of what was written into the vectors."""
    dev, nx = params.device, params.N[0]
    pipe = _Pipeline(params, len(names), band_rows)
    item = params.data_type.itemsize
    try:
        for k, (r0, rows) in enumerate(pipe.bands):
            s = k & 1
            if k >= 2:
                dev.event_sync(BAND_EVENT_SLOT + s)       # band k - 2 has left this pair of buffers
            band = pipe.host[s].array.view(np.uint8)
            for q in range(len(names)):
                for off, n, at in _file_runs(params, names, q, r0, rows):
                    lo = (q * rows * nx + at) * item
                    got = os.preadv(fd, [memoryview(band[lo:lo + n * item])], off)
                    if got != n * item:
                        solver_error("io", f"truncated checkpoint: {got} of {n * item} bytes at offset {off}")
            pipe.host[s].copy_to_device_async(pipe.stage[s], n=len(names) * rows * nx)
            _move(params, grid, names, (0, r0, nx, rows), pipe.stage[s], pipe.digest, unpack=True)
            dev.event_record(BAND_EVENT_SLOT + s)
        return pipe.digests()
    finally:
        pipe.free()


# ---- packed files: the index, the reader, the writer ---------------------------------------------------------------------
def _io(path, what):
    solver_error("io", f"{path}: {what}")


def check_index(path, header, records, mask_table=None):
    """Validate the index ``records`` (``[count][8]`` integers) of the packed file ``path`` against its header: every record
    lies inside the chunk area and none overlaps another, windows lie inside the domain, the chunks of each plane tile
    ``[NY][NX]`` exactly, the planes of a saved band share its window, and the length of every encoded chunk is the one its
    mask table gives (``mask_table(offset, nbytes)`` → that many bytes of the file; None = not looked at). Any failure is an
    I/O error that names the file → the saved bands ``[(window, {plane: record})]`` in file order, ``window`` = global
    ``(col0, row0, wnx, wny)``."""
    NX, NY = header["N"]
    item = np.dtype(header["data_type"]).itemsize
    nplanes, end = len(header["planes"]), header["index_offset"]
    records = [tuple(int(v) for v in r) for r in records]
    for rec in records:
        q, codec, col0, row0, wnx, wny, off, nbytes = rec
        if q >= nplanes or codec not in (CODEC_RAW, CODEC_XORPLANE):
            _io(path, f"damaged index: plane {q}, codec {codec}")
        if wnx < 1 or wny < 1 or col0 + wnx > NX or row0 + wny > NY:
            _io(path, f"damaged index: the window [{col0}, {col0 + wnx}) x [{row0}, {row0 + wny}) leaves the domain {NX} x {NY}")
        if off < DATA_OFFSET or off % 8 or off + nbytes > end:
            _io(path, f"damaged index: a chunk of {nbytes} bytes at offset {off} leaves the chunk area [{DATA_OFFSET}, {end})")
        if codec == CODEC_RAW and nbytes != wnx * wny * item:
            _io(path, f"damaged index: a raw chunk of {wnx} x {wny} with {nbytes} bytes")
        if codec == CODEC_XORPLANE and not 2 * plane_codec.table_bytes(wny, wnx, item) <= nbytes <= plane_codec.bound(wny, wnx, item):
            _io(path, f"damaged index: an encoded chunk of {wnx} x {wny} with {nbytes} bytes")
    by_offset = sorted(records, key=lambda r: r[6])
    for a, b in zip(by_offset, by_offset[1:]):
        if a[6] + a[7] > b[6]:
            _io(path, f"damaged index: the chunks at offsets {a[6]} and {b[6]} overlap")
    for q in range(nplanes):
        mine = [r for r in records if r[0] == q]
        xs = sorted({r[2] for r in mine} | {r[2] + r[4] for r in mine} | {0, NX})
        ys = sorted({r[3] for r in mine} | {r[3] + r[5] for r in mine} | {0, NY})
        xi, yi = {x: i for i, x in enumerate(xs)}, {y: i for i, y in enumerate(ys)}
        cover = np.zeros((len(ys) - 1, len(xs) - 1), dtype=np.int64)      # the domain cut at every edge of a window
        for r in mine:
            cover[yi[r[3]]:yi[r[3] + r[5]], xi[r[2]]:xi[r[2] + r[4]]] += 1
        if (cover != 1).any():
            iy, ix = np.argwhere(cover != 1)[0]
            _io(path, f"damaged index: the chunks of plane {header['planes'][q]} {'overlap' if cover[iy, ix] else 'leave a hole'} "
                      f"at cell ({xs[ix]}, {ys[iy]})")
    bands = {}
    for rec in by_offset:
        bands.setdefault(rec[2:6], {})[rec[0]] = rec
    if any(len(planes) != nplanes for planes in bands.values()):
        _io(path, "damaged index: the planes of a saved band do not share its window")
    if mask_table is not None:
        for q, codec, col0, row0, wnx, wny, off, nbytes in by_offset:
            if codec == CODEC_XORPLANE:
                table = plane_codec.table_bytes(wny, wnx, item)
                masks = np.frombuffer(mask_table(off + table, table), dtype=np.uint8)[:plane_codec.groups(wny, wnx)[1] * item]
                want = plane_codec.chunk_size(masks.view("<u8" if item == 8 else "<u4"))
                if want != nbytes:
                    _io(path, f"damaged chunk at offset {off}: its mask table asks for {want} bytes, the index says {nbytes}")
    return list(bands.items())


def read_index(path, header, fd=None):
    """The validated saved bands of the packed checkpoint ``path`` (``check_index``), mask tables included."""
    own = fd is None
    try:
        if own:
            fd = os.open(path, os.O_RDONLY)
        try:
            def pread(offset, nbytes):
                data = os.pread(fd, nbytes, offset)
                if len(data) != nbytes:
                    _io(path, f"truncated checkpoint: {len(data)} of {nbytes} bytes at offset {offset}")
                return data
            raw = pread(header["index_offset"], INDEX_RECORD * header["index_count"])
            return check_index(path, header, np.frombuffer(raw, dtype="<u8").reshape(-1, 8), pread)
        finally:
            if own:
                os.close(fd)
    except OSError as e:
        solver_error("io", f"cannot read the checkpoint {path}: {e}")


def _cut(params, window):
    """The cells the tile shares with the global ``window`` → global (x0, y0, snx, sny), or None."""
    ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
    x0, y0 = max(ox, window[0]), max(oy, window[1])
    x1, y1 = min(ox + params.N[0], window[0] + window[2]), min(oy + params.N[1], window[1] + window[3])
    return (x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else None


def _readinto(fd, view, offset, path):
    got = os.preadv(fd, [view], offset)
    if got != len(view):
        _io(path, f"truncated checkpoint: {got} of {len(view)} bytes at offset {offset}")


def packed_pieces(fd, path, header, bands, params, names, want=None):
    """THE reader of packed files, for ``load`` and ``compare_state``: for every saved band that intersects this tile (and that
    ``want(window)`` does not turn down) read the chunks of the planes ``names``, copy them to the device, decode the
    intersection of each (``armon_hip_plane_decode``; a raw chunk is cut on the host) → yields ``(window, dense)``: the
    intersection as a window ``(col0, row0, snx, sny)`` of the tile's real cells and the device array ``[len(names)][sny][snx]``
    that holds it, valid until the next piece is asked for. One piece is in flight at a time."""
    dev, dtype = params.device, params.data_type
    item = dtype.itemsize
    ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
    planes = [header["planes"].index(f) for f in names]
    work = []
    for window, recs in bands:
        cut = _cut(params, window)
        if cut is not None and (want is None or want((cut[0] - ox, cut[1] - oy, cut[2], cut[3]))):
            work.append((window, [recs[q] for q in planes], cut))
    if not work:
        return
    chunk_bytes = max(sum(plane_codec.pad8(r[7]) for r in recs if r[1] == CODEC_XORPLANE) for _, recs, _ in work)
    cells = max(len(names) * cut[2] * cut[3] for _, _, cut in work)
    bufs = []
    try:
        dense, status = dev.empty(cells, dtype), dev.zeros(2, np.uint32)
        bufs += [dense, status]
        host = dev.pinned(cells, dtype)
        bufs.append(host)
        chunks = chunks_host = None
        if chunk_bytes:
            chunks, chunks_host = dev.empty(chunk_bytes, np.uint8), dev.pinned(chunk_bytes, np.uint8)
            bufs += [chunks, chunks_host]
        decode = params.fn("plane_decode")
        for (col0, row0, wnx, wny), recs, (x0, y0, snx, sny) in work:
            params.wait()                                       # the piece before has left the buffers
            at = 0
            for k, (q, codec, _, _, _, _, off, nbytes) in enumerate(recs):
                if codec == CODEC_RAW:
                    out = host.array.view(np.uint8)[k * sny * snx * item:(k + 1) * sny * snx * item]
                    first = off + ((y0 - row0) * wnx + x0 - col0) * item
                    if snx == wnx:
                        _readinto(fd, memoryview(out), first, path)
                    else:
                        for r in range(sny):
                            _readinto(fd, memoryview(out[r * snx * item:(r + 1) * snx * item]), first + r * wnx * item, path)
                    host.copy_to_device_async(dense, n=sny * snx, src_offset=k * sny * snx, dst_offset=k * sny * snx)
                else:
                    _readinto(fd, memoryview(chunks_host.array[at:at + nbytes]), off, path)
                    chunks_host.copy_to_device_async(chunks, n=nbytes, src_offset=at, dst_offset=at)
                    check(decode(dev.ctx, C.c_void_p(chunks.ptr + at), nbytes, wny, wnx, x0 - col0, y0 - row0, snx, sny,
                                 C.c_void_p(dense.ptr + k * sny * snx * item), C.c_void_p(status.ptr)))
                    at += plane_codec.pad8(nbytes)
            yield (x0 - ox, y0 - oy, snx, sny), dense
        params.wait()
        if status.to_host()[0]:
            _io(path, "damaged chunk: the words of a group end past the chunk")
    finally:
        params.wait()
        for a in bufs:
            a.free()


def _save_tile_packed(fd, params, grid, names, band_rows, offset, records):
    """Pack, encode, copy and write the bands of one tile as chunks from the file offset ``offset`` on; their index records
    join ``records`` → (the tile's per-plane digests, the offset after its last chunk). Per band: state_pack into the staging
    buffer (the digest is that of an unpacked save), plane_encode into a second device buffer; the sizes are read back after
    the band's event, and only the used bytes — of the encoding, or of the staging buffer where the encoding is not smaller —
    are copied to pinned memory and written while the next band is packed and encoded. Stream order keeps one buffer of each
    kind safe: the copies of band k are queued before the kernels of band k + 1."""
    dev, nx, item = params.device, params.N[0], params.data_type.itemsize
    ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
    nvars = len(names)
    rows_max, bands = _bands(params, nvars, band_rows)
    bound = plane_codec.bound(rows_max, nx, item)
    encode = params.fn("plane_encode")
    bufs = []
    try:
        digest = dev.zeros(8, np.uint64)
        bufs.append(digest)
        stage = dev.empty(nvars * rows_max * nx, params.data_type)
        bufs.append(stage)
        enc = dev.empty(nvars * bound, np.uint8)
        bufs.append(enc)
        sizes = dev.zeros(8, np.uint64)
        bufs.append(sizes)
        sizes_host = dev.pinned(8, np.uint64)
        bufs.append(sizes_host)
        host = dev.pinned(nvars * rows_max * nx * item, np.uint8)
        bufs.append(host)

        def launch(k):
            r0, rows = bands[k]
            _move(params, grid, names, (0, r0, nx, rows), stage, digest)
            check(encode(dev.ctx, C.c_void_p(stage.ptr), nvars, rows, nx, C.c_void_p(enc.ptr), bound, C.c_void_p(sizes.ptr)))
            sizes_host.copy_from_device_async(sizes, n=nvars)
            dev.event_record(BAND_EVENT_SLOT)

        def fetch(k):
            """Queue the copies of band k's used bytes → [(codec, bytes)] per plane."""
            r0, rows = bands[k]
            raw = rows * nx * item
            dev.event_sync(BAND_EVENT_SLOT)
            out = []
            for q in range(nvars):
                n = int(sizes_host.array[q])
                codec, src = (CODEC_XORPLANE, enc.ptr + q * bound) if n < raw else (CODEC_RAW, stage.ptr + q * raw)
                n = min(n, raw)
                check(dev._L.armon_hip_memcpy_async(dev.ctx, C.c_void_p(host.ptr + q * raw), C.c_void_p(src), n, 2))
                out.append((codec, n))
            dev.event_record(BAND_EVENT_SLOT + 1)
            return out

        def flush(k, chunks):
            nonlocal offset
            r0, rows = bands[k]
            raw = rows * nx * item
            dev.event_sync(BAND_EVENT_SLOT + 1)
            for q, (codec, n) in enumerate(chunks):
                _pwrite_all(fd, memoryview(host.array[q * raw:q * raw + n]), offset)
                records.append((q, codec, ox, oy + r0, nx, rows, offset, n))
                offset += plane_codec.pad8(n)

        launch(0)
        for k in range(1, len(bands)):
            chunks = fetch(k - 1)
            launch(k)                                   # runs while band k - 1 is written
            flush(k - 1, chunks)
        flush(len(bands) - 1, fetch(len(bands) - 1))
        params.wait()
        return [int(v) for v in digest.to_host()[:nvars]], offset
    finally:
        params.wait()
        for a in bufs:
            a.free()


def _load_tile_packed(fd, path, header, bands, params, grid, names):
    """Every saved band that intersects the tile: decode the intersection, one state_unpack of it (the variable index k of
    the digest is the plane's) → the per-plane digests of what was written into the vectors."""
    dev = params.device
    digest = dev.zeros(8, np.uint64)
    try:
        for window, dense in packed_pieces(fd, path, header, bands, params, names):
            _move(params, grid, names, window, dense, digest, unpack=True)
        params.wait()
        return [int(v) for v in digest.to_host()[:len(names)]]
    finally:
        params.wait()
        digest.free()


def expand(src, dst):
    """The packed checkpoint ``src`` as the version-1 file ``dst`` of the same state: the same header without the keys of a
    packed file, the dense planes. Host only (numpy): no device is touched, no digest computed → the header written."""
    src, dst = str(src), str(dst)
    header = read_header(src)
    if not is_packed(header):
        solver_error("io", f"{src} is not a packed checkpoint")
    NX, NY = header["N"]
    dtype = np.dtype(header["data_type"])
    item = dtype.itemsize
    plain = {k: v for k, v in header.items() if k not in PACKED_KEYS}
    tmp = dst + ".tmp"
    try:
        fd = os.open(src, os.O_RDONLY)
        try:
            bands = read_index(src, header, fd)
            out = os.open(tmp, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                os.ftruncate(out, DATA_OFFSET + len(header["planes"]) * NX * NY * item)
                for (col0, row0, wnx, wny), recs in bands:
                    for q, codec, _, _, _, _, off, nbytes in recs.values():
                        data = os.pread(fd, nbytes, off)
                        if len(data) != nbytes:
                            _io(src, f"truncated checkpoint: {len(data)} of {nbytes} bytes at offset {off}")
                        try:
                            plane = (plane_codec.decode_reference(data, wny, wnx, dtype) if codec == CODEC_XORPLANE
                                     else np.frombuffer(data, dtype=dtype).reshape(wny, wnx))
                        except ValueError as e:
                            _io(src, f"damaged chunk at offset {off}: {e}")
                        first = DATA_OFFSET + ((q * NY + row0) * NX + col0) * item
                        if wnx == NX:
                            _pwrite_all(out, plane.tobytes(), first)
                        else:
                            for r in range(wny):
                                _pwrite_all(out, plane[r].tobytes(), first + r * NX * item)
                with os.fdopen(os.dup(out), "r+b") as f:
                    write_header(f, plain)
                    f.flush()
                os.fsync(out)
            finally:
                os.close(out)
        finally:
            os.close(fd)
        os.replace(tmp, dst)
    except BaseException as e:
        if os.path.exists(tmp):
            os.unlink(tmp)
        if isinstance(e, OSError):
            solver_error("io", f"cannot expand the checkpoint {src} into {dst}: {e}")
        raise
    return plain


# ---- a whole run ---------------------------------------------------------------------------------------------------------
def _refuse_ranks(params):
    if params.use_MPI:
        solver_error("config", "checkpoint / restart is not supported for ranks of a process group (use_MPI=true)")


def save(tiles, gdt, readback, path, band_rows=None, compress=None):
    """Write the checkpoint ``path`` of the run whose tiles are the ``(params, grid)`` of ``tiles`` (idle, nothing in flight
    between them), at the boundary before cycle ``gdt.cycle`` → the header. ``readback`` = the run's ``DtReadback``: the CFL
    step the previous cycle left in flight (fused path) is taken, stored, and primed again exactly as a restart primes it, so
    that writing a checkpoint cannot change the run's bits. Written as ``path.tmp``, then renamed. ``compress``: write a packed
    file (None = the ``checkpoint_compress`` option); without it the file is version 1, byte for byte what it always was."""
    p0 = tiles[0][0]
    _refuse_ranks(p0)
    compress = bool(getattr(p0, "checkpoint_compress", False) if compress is None else compress)
    names = plane_names(p0)
    pending = None
    if (gdt.cycle - 1) in readback.inflight:
        pending = readback.take(gdt.cycle - 1)
        readback.prime(gdt.cycle - 1, pending)
    NX, NY = p0.global_grid
    header = dict(bit_options(p0))
    header.update(version=VERSION, planes=list(names), cycle=int(gdt.cycle), time=hexfloat(gdt.time),
                  current_dt=hexfloat(gdt.current_dt), next_cycle_dt=hexfloat(gdt.next_cycle_dt),
                  pending_dt=None if pending is None else hexfloat(pending))
    if p0.initial_mass != 0 or p0.initial_energy != 0:
        header.update(initial_mass=hexfloat(p0.initial_mass), initial_energy=hexfloat(p0.initial_energy))
    path = str(path)
    tmp = path + ".tmp"
    total = [0] * len(names)
    try:
        # like every other output (io.build_file_path): the directory is made on first need
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        fd = os.open(tmp, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644)
    except OSError as e:
        solver_error("io", f"cannot create the checkpoint {path}: {e}")
    try:
        if compress:
            offset, records = DATA_OFFSET, []
            for params, grid in tiles:
                digests, offset = _save_tile_packed(fd, params, grid, names, band_rows, offset, records)
                total = [(t + d) & MASK for t, d in zip(total, digests)]
            _pwrite_all(fd, np.array(records, dtype="<u8").tobytes(), offset)
            os.ftruncate(fd, offset + INDEX_RECORD * len(records))
            header.update(codec=CODEC, index_offset=offset, index_count=len(records))
        else:
            os.ftruncate(fd, DATA_OFFSET + len(names) * NX * NY * p0.data_type.itemsize)
            for params, grid in tiles:
                total = [(t + d) & MASK for t, d in zip(total, _save_tile(fd, params, grid, names, band_rows))]
        header["digests"] = {f: f"{d:016x}" for f, d in zip(names, total)}
        with os.fdopen(os.dup(fd), "r+b") as f:
            write_header(f, header, VERSION_PACKED if compress else VERSION)
            f.flush()
        os.fsync(fd)
        os.close(fd)
        fd = -1
        os.replace(tmp, path)
    except BaseException as e:
        if fd >= 0:
            os.close(fd)
        if os.path.exists(tmp):
            os.unlink(tmp)
        if isinstance(e, OSError):
            solver_error("io", f"cannot write the checkpoint {path}: {e}")
        raise
    return header


def load(tiles, gdt, readback, path, band_rows=None):
    """Load the checkpoint ``path`` over the initialised tiles of a run: the state planes (and ``c`` on the staged path), the
    clock, and the pending CFL step, primed so that the next cycle is "deferred" and finds it → the header. The digests
    accumulated while writing the vectors are compared with the header's."""
    p0 = tiles[0][0]
    _refuse_ranks(p0)
    header = read_header(path)
    check_compatible(p0, header, path)
    names = tuple(header["planes"])
    if names != plane_names(p0):
        solver_error("config", f"the checkpoint {path} holds the planes {names}, this run needs {plane_names(p0)}")
    total = [0] * len(names)
    try:
        fd = os.open(path, os.O_RDONLY)
        try:
            bands = read_index(path, header, fd) if is_packed(header) else None     # validated before anything goes to a device
            for params, grid in tiles:
                digests = (_load_tile(fd, params, grid, names, band_rows) if bands is None
                           else _load_tile_packed(fd, str(path), header, bands, params, grid, names))
                total = [(t + d) & MASK for t, d in zip(total, digests)]
        finally:
            os.close(fd)
    except OSError as e:
        solver_error("io", f"cannot read the checkpoint {path}: {e}")
    for f, d in zip(names, total):
        if f"{d:016x}" != header["digests"][f]:
            solver_error("io", f"{path}: digest mismatch in plane {f}: the header says {header['digests'][f]}, "
                               f"the data gives {d:016x}")
    T = p0.T
    gdt.cycle = int(header["cycle"])
    gdt.time, gdt.current_dt = T(unhex(header["time"])), T(unhex(header["current_dt"]))
    gdt.next_cycle_dt = T(unhex(header["next_cycle_dt"]))
    readback.inflight.clear()
    if header["pending_dt"] is not None:
        readback.prime(gdt.cycle - 1, T(unhex(header["pending_dt"])))
    for params, grid in tiles:
        if "initial_mass" in header:
            params.initial_mass, params.initial_energy = unhex(header["initial_mass"]), unhex(header["initial_energy"])
        grid.initialised = True
        if params.use_fused_sweep:
            grid.release_scratch()               # nothing reads c, g after cycle 0
    return header
