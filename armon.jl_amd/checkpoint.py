"""Checkpoint and bit-exact restart, with a state digest computed on the device (csrc/checkpoint.hip). No reference
counterpart: the reference's only state files are text at ``output_precision`` (ref src/io.jl:2-27).

File, in this order: the magic ``ARMONCKP``, a u32 version, a u32 header length, a UTF-8 JSON header padded with spaces to
4096 bytes, then the dense GLOBAL planes ``[NY][NX]`` of real cells, little-endian, in the order rho, u, v, E — and ``c`` as a
fifth plane when the run is staged (its ``next_time_step`` reads the ``c`` the last EOS of the previous cycle left). Ghost
cells are not stored: both paths rebuild them before any read.

The digest of plane k is the sum mod 2^64 over its cells of ``mix64(b + mix64(8 g + k + 1))`` — ``b`` the value's bit pattern
zero-extended to 64 bits, ``g = gy NX + gx`` its global 0-based index, ``mix64`` as in ``mix64`` below. It depends on the
values and their global positions only, so the tiles of a group add their digests up to the single block's.

Pipeline: a tile's window is cut into row bands; band k is packed (and digested) into one of two device staging buffers,
copied asynchronously into one of two pinned host buffers, and written at its file offset while band k + 1 is being packed.
Host and staging memory are 2 x band, never a whole field. The band height comes from a byte budget of 256 MB per buffer —
large enough that a band's kernel and copy (tens of ms) dwarf their launch cost, small enough to be pinned without a thought
next to a 16384² run (8.6 GB per plane) — or from ``band_rows``. Restore runs the same bands the other way.
"""
import ctypes as C
import json
import os
import struct

import numpy as np

from ._lib import check, solver_error

MAGIC = b"ARMONCKP"
VERSION = 1
HEADER_BYTES = 4096                       # the JSON header, padded
DATA_OFFSET = len(MAGIC) + 4 + 4 + HEADER_BYTES
BAND_BYTES = 256 << 20                    # per staging / pinned buffer
BAND_EVENT_SLOT = 1016                    # event-pool slots 1016, 1017: one per staging buffer
STATE_PLANES = ("rho", "u", "v", "E")
MASK = (1 << 64) - 1

# every option that decides bits: a restart must agree with the file on all of them
BIT_FIELDS = ("data_type", "N", "test", "domain_size", "origin", "periodic", "scheme", "riemann_limiter", "projection", "axis_splitting",
              "eos", "cfl", "cst_dt", "Dt", "use_fused_sweep", "exact_arithmetic")


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


def write_header(f, header):
    """The preamble at offset 0 of the open binary file ``f``: magic, version, header length, padded JSON."""
    text = json.dumps(header, sort_keys=True).encode("utf-8")
    if len(text) > HEADER_BYTES:
        solver_error("io", f"checkpoint header of {len(text)} bytes does not fit in {HEADER_BYTES}")
    f.seek(0)
    f.write(MAGIC + struct.pack("<II", VERSION, len(text)) + text + b" " * (HEADER_BYTES - len(text)))


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
    if version != VERSION:
        solver_error("io", f"{path}: checkpoint version {version}, this build reads version {VERSION}")
    if length > HEADER_BYTES or len(pre) < DATA_OFFSET:
        solver_error("io", f"{path}: truncated or damaged header")
    try:
        header = json.loads(pre[16:16 + length].decode("utf-8"))
    except ValueError as e:
        solver_error("io", f"{path}: unreadable header: {e}")
    _check_header(header, path)
    NX, NY = header["N"]
    want = DATA_OFFSET + len(header["planes"]) * NX * NY * np.dtype(header["data_type"]).itemsize
    if size != want:
        solver_error("io", f"{path}: truncated checkpoint: {size} bytes, {want} expected")
    return header


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
    if ("initial_mass" in header or "initial_energy" in header) and not (
            _is_hexfloat(header.get("initial_mass")) and _is_hexfloat(header.get("initial_energy"))):
        bad("initial_mass / initial_energy")


def bit_options(params):
    """What decides the bits of a run, as the header stores it (floats as hex text)."""
    fused = bool(params.use_fused_sweep)
    return {"data_type": params.data_type.name, "N": list(params.global_grid),
            "domain_size": [hexfloat(v) for v in params.domain_size], "origin": [hexfloat(v) for v in params.origin],
            "periodic": [bool(v) for v in params.periodic], "test": params.test.name, "scheme": params.riemann_scheme, "riemann_limiter": params.riemann_limiter,
            "projection": params.projection_scheme, "axis_splitting": params.axis_splitting, "eos": params.test.eos,
            "cfl": hexfloat(params.cfl), "cst_dt": bool(params.cst_dt), "Dt": hexfloat(params.Dt),
            "use_fused_sweep": fused, "exact_arithmetic": bool(params.exact_arithmetic) if fused else None}


def check_compatible(params, header, path):
    """A configuration error that names the first bit-deciding field on which the file and the run disagree, or a file that
    leaves nothing to run. ``nghost``, the decomposition, ``maxcycle``, ``maxtime`` and the output options are free."""
    mine = bit_options(params)
    for k in BIT_FIELDS:
        if header.get(k) != mine[k]:
            solver_error("config", f"the checkpoint {path} was written with {k} = {header.get(k)!r}, this run has "
                                   f"{k} = {mine[k]!r}")
    if header["cycle"] >= params.maxcycle or params.T(unhex(header["time"])) >= params.T(params.maxtime):
        solver_error("config", f"the checkpoint {path} is at cycle {header['cycle']}, time {unhex(header['time'])}: nothing left "
                               f"to run with maxcycle = {params.maxcycle}, maxtime = {params.maxtime}")


def checkpoint_path(params, cycle):
    return os.path.join(params.output_dir, f"{params.checkpoint_file}_{cycle:06d}.ckpt")


def plane_names(params):
    return STATE_PLANES + (() if params.use_fused_sweep else ("c",))


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


# ---- a whole run ---------------------------------------------------------------------------------------------------------
def _refuse_ranks(params):
    if params.use_MPI:
        solver_error("config", "checkpoint / restart is not supported for ranks of a process group (use_MPI=true)")


def save(tiles, gdt, readback, path, band_rows=None):
    """Write the checkpoint ``path`` of the run whose tiles are the ``(params, grid)`` of ``tiles`` (idle, nothing in flight
    between them), at the boundary before cycle ``gdt.cycle`` → the header. ``readback`` = the run's ``DtReadback``: the CFL
    step the previous cycle left in flight (fused path) is taken, stored, and primed again exactly as a restart primes it, so
    that writing a checkpoint cannot change the run's bits. Written as ``path.tmp``, then renamed."""
    p0 = tiles[0][0]
    _refuse_ranks(p0)
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
        os.ftruncate(fd, DATA_OFFSET + len(names) * NX * NY * p0.data_type.itemsize)
        for params, grid in tiles:
            total = [(t + d) & MASK for t, d in zip(total, _save_tile(fd, params, grid, names, band_rows))]
        header["digests"] = {f: f"{d:016x}" for f, d in zip(names, total)}
        with os.fdopen(os.dup(fd), "r+b") as f:
            write_header(f, header)
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
            for params, grid in tiles:
                total = [(t + d) & MASK for t, d in zip(total, _load_tile(fd, params, grid, names, band_rows))]
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
