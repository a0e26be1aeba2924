"""Text output / input in the reference's file format, and the per-step comparison against dumps.

Mirrors ref src/io.jl: ``write_blocks_to_file`` (:3-27, one line ``x, y, ρ, u, v, p`` per cell in ascending
(x, y) order, ``%#{p+7}.{p}e`` fields joined by ", ", a blank line between rows for gnuplot's pm3d),
``read_data_from_file`` (:30-43), ``build_file_path`` (:44-58, ``_{cx}×{cy}`` suffix per sub-domain),
``write/read_time_step_file`` (:84-105) and ``step_checkpoint`` / ``compare_with_file`` (:113-227) which dump
or diff every sub-step of the staged solver cycle (``compare`` / ``is_ref`` options). The golden files of
ref test/reference_data use the same cell format after a ``dt, cycles`` header line
(ref test/reference_data/reference_functions.jl:37-50).
"""
import os

import numpy as np

SAVED_VARS = ("x", "y", "rho", "u", "v", "p")      # ref src/blocking/blocks.jl:49


def _fmt(precision):
    return f"%#{precision + 7}.{precision}e"


def build_file_path(params, file_name):
    path = os.path.join(params.output_dir, file_name)
    if params.is_root and not os.path.isdir(params.output_dir):
        os.makedirs(params.output_dir, exist_ok=True)
    if params.use_MPI:
        path += "_" + "×".join(str(c) for c in params.cart_coords)
    return path


def _rows(params, ghosts):
    """(first, last) 0-based array indices of the rows / columns written (ghosts only where the tile
    touches the global boundary, like the reference's ``global_ghosts``)."""
    g = params.nghost
    nx, ny = params.N
    if not ghosts:
        return (g, g + nx), (g, g + ny)
    P, cc = params.proc_dims, params.cart_coords
    x0 = 0 if cc[0] == 0 else g
    x1 = nx + 2 * g if cc[0] == P[0] - 1 else g + nx
    y0 = 0 if cc[1] == 0 else g
    y1 = ny + 2 * g if cc[1] == P[1] - 1 else g + ny
    return (x0, x1), (y0, y1)


def write_blocks_to_file(params, host, file, vars=SAVED_VARS, global_ghosts=False, for_3D=True):
    """``host`` = dict name → flat ghosted numpy array (``BlockGrid.device_to_host()``)."""
    fmt = ", ".join([_fmt(params.output_precision)] * len(vars)) + "\n"
    sx = params.N[0] + 2 * params.nghost
    (x0, x1), (y0, y1) = _rows(params, global_ghosts)
    cols = [np.asarray(host[v]).reshape(-1, sx) for v in vars]
    for j in range(y0, y1):
        if j != y0 and for_3D:
            file.write("\n")                      # separate rows to use pm3d plotting with gnuplot
        rows = [c[j, x0:x1] for c in cols]
        file.write("".join(fmt % vals for vals in zip(*rows)))


def read_data_from_file(params, host, file, vars=SAVED_VARS, global_ghosts=False):
    sx = params.N[0] + 2 * params.nghost
    (x0, x1), (y0, y1) = _rows(params, global_ghosts)
    vals = np.array([[float(t) for t in line.split(",")] for line in file if line.strip()], dtype=np.float64)
    expected = (x1 - x0) * (y1 - y0)
    if vals.shape != (expected, len(vars)):
        raise ValueError(f"expected {expected} lines of {len(vars)} values, found an array of shape {vals.shape}")
    vals = vals.reshape(y1 - y0, x1 - x0, len(vars))
    for k, v in enumerate(vars):
        np.asarray(host[v]).reshape(-1, sx)[y0:y1, x0:x1] = vals[:, :, k]


def write_sub_domain_file(params, grid, file_name, no_msg=False, vars=SAVED_VARS, coarse=False):
    """``coarse=True`` (what ``armon`` and the animation frames pass when ``output_coarsen`` is set): the file holds the
    state coarsened on the device, see ``write_coarse_file``; no full field goes to the host."""
    if coarse:
        path = write_coarse_file(params, grid.coarsen(params.output_coarsen), file_name)
    else:
        path = build_file_path(params, file_name)
        host = grid.device_to_host(vars)
        with open(path, "w") as f:
            write_blocks_to_file(params, host, f, vars=vars, global_ghosts=params.write_ghosts)
    if not no_msg and params.is_root and params.silent < 2:
        print(f"\nWrote to files {path}_*x*")
    return path


def write_coarse_planes_to_file(params, planes, file, vars=SAVED_VARS):
    """``planes`` = dict name → ``(cny, cnx)`` array (``BlockGrid.coarsen``): one line per coarse cell in the cell format of
    ``write_blocks_to_file`` (``x, y, ρ, u, v, p``, ``output_precision``), a blank line between coarse rows."""
    fmt = ", ".join([_fmt(params.output_precision)] * len(vars)) + "\n"
    cols = [np.asarray(planes[v]) for v in vars]
    for j in range(cols[0].shape[0]):
        if j != 0:
            file.write("\n")
        file.write("".join(fmt % vals for vals in zip(*[c[j] for c in cols])))


def write_coarse_file(params, planes, file_name, vars=SAVED_VARS):
    path = build_file_path(params, file_name)
    with open(path, "w") as f:
        write_coarse_planes_to_file(params, planes, f, vars=vars)
    return path


def read_coarse_file(params, file_name, vars=SAVED_VARS):
    """Reads a file of ``write_coarse_file`` back → dict name → ``(cny, cnx)`` float64 array. The shape comes from the file
    itself: blank lines separate the coarse rows."""
    rows, row = [], []
    with open(build_file_path(params, file_name)) as f:
        for line in f:
            if line.strip():
                row.append([float(t) for t in line.split(",")])
            elif row:
                rows.append(row)
                row = []
    if row:
        rows.append(row)
    if not rows or any(len(r) != len(rows[0]) for r in rows) or any(len(c) != len(vars) for r in rows for c in r):
        raise ValueError(f"{file_name}: not a coarse file of {len(vars)} values per line in rows of equal length")
    vals = np.array(rows, dtype=np.float64)
    return {v: vals[:, :, k] for k, v in enumerate(vars)}


def write_slices_files(params, grid, file_name, vars=SAVED_VARS):
    """``write_slices=true`` (ref src/parameters.jl:229-232, call at src/solver.jl:508): "all saved_vars() to 3 output
    files, one for the middle X row, another for the middle Y column, and another for the diagonal; with write_ghosts the
    ghost cells too". The reference calls ``write_slices_files`` but does not define it anywhere in src/, so the file
    names are this backend's: ``<file>_X`` (the row j = Ny÷2), ``<file>_Y`` (the column i = Nx÷2), ``<file>_diag`` (cells
    (k, k), k < min(Nx, Ny)), each in the cell format of ``write_blocks_to_file``. Single block only (a tile writes the
    slices of its own sub-domain, with the sub-domain suffix of ``build_file_path``). The cells are picked on the device
    (``BlockGrid.gather``: stride 1 along the row, the row pitch along the column, pitch + 1 along the diagonal): three
    lines of cells cross PCIe, not six fields."""
    fmt = ", ".join([_fmt(params.output_precision)] * len(vars)) + "\n"
    sx = params.N[0] + 2 * params.nghost
    g = params.nghost
    (x0, x1), (y0, y1) = _rows(params, params.write_ghosts)
    jm, im = g + params.N[1] // 2, g + params.N[0] // 2
    n_diag = min(x1 - x0, y1 - y0)
    picks = {"X": (jm * sx + x0, 1, x1 - x0), "Y": (y0 * sx + im, sx, y1 - y0), "diag": (y0 * sx + x0, sx + 1, n_diag)}
    paths = []
    for tag, (start, stride, count) in picks.items():
        cells = grid.gather(vars, start, stride, count)
        path = build_file_path(params, f"{file_name}_{tag}")
        with open(path, "w") as f:
            f.write("".join(fmt % vals for vals in zip(*[cells[v] for v in vars])))
        paths.append(path)
    if params.is_root and params.silent < 2:
        print(f"\nWrote slices to {', '.join(paths)}")
    return paths


def prepare_animation_dir(params):
    """ref src/solver.jl:436-442: the root empties (or creates) the ``anim`` directory before the run."""
    if params.animation_step == 0 or not params.is_root:
        return
    d = os.path.join(params.output_dir, "anim")
    if os.path.isdir(d):
        for name in os.listdir(d):
            os.remove(os.path.join(d, name))
    else:
        os.makedirs(d)


def write_animation_frame(params, grid):
    """ref src/solver.jl:373-378, called after ``next_cycle!``: every ``animation_step`` cycles the saved_vars go to
    ``anim/<output_file>_<frame:03d>`` as with write_output."""
    cycle = grid.global_dt.cycle
    if params.animation_step == 0 or (cycle - 1) % params.animation_step != 0:
        return None
    frame = (cycle - 1) // params.animation_step
    return write_sub_domain_file(params, grid, os.path.join("anim", params.output_file) + f"_{frame:03d}", no_msg=True,
                                 coarse=params.output_coarsen is not None)


def read_sub_domain_file(params, file_name, vars=SAVED_VARS):
    """Returns dict name → flat ghosted array (cells not in the file are NaN)."""
    n = params.block_size.n_cells
    host = {v: np.full(n, np.nan) for v in vars}
    with open(build_file_path(params, file_name)) as f:
        read_data_from_file(params, host, f, vars=vars, global_ghosts=params.write_ghosts)
    return host


def write_time_step_file(params, dt, file_name):
    with open(build_file_path(params, file_name), "w") as f:
        f.write(_fmt(params.output_precision) % dt + "\n")


def read_time_step_file(params, file_name):
    with open(build_file_path(params, file_name)) as f:
        return float(f.read().strip())


def read_reference_file(path, N):
    """A golden file of ref test/reference_data: header ``dt, cycles`` then the saved_vars of the real cells.
    Returns (dt, cycles, dict name → (Ny, Nx) array)."""
    with open(path) as f:
        head = f.readline().split(",")
        vals = np.array([[float(t) for t in line.split(",")] for line in f if line.strip()])
    vals = vals.reshape(N[1], N[0], len(SAVED_VARS))
    return float(head[0]), int(head[1]), {v: vals[:, :, k] for k, v in enumerate(SAVED_VARS)}


def write_reference_file(params, grid, dt, cycles, path):
    """ref test/reference_data/reference_functions.jl:37-43"""
    host = grid.device_to_host(SAVED_VARS)
    with open(path, "w") as f:
        f.write("%#.15g, %d\n" % (dt, cycles))
        write_blocks_to_file(params, host, f)


# ---- comparison (ref src/io.jl:113-227) -------------------------------------------------------------------
def compare_host(params, ref, ours, label, vars=SAVED_VARS, verbose=True):
    """True when ``ours`` differs from ``ref`` beyond ``comparison_tolerance`` (relative), real cells only
    unless write_ghosts."""
    sx = params.N[0] + 2 * params.nghost
    (x0, x1), (y0, y1) = _rows(params, params.write_ghosts)
    different = False
    for v in vars:
        a = np.asarray(ref[v]).reshape(-1, sx)[y0:y1, x0:x1]
        b = np.asarray(ours[v]).reshape(-1, sx)[y0:y1, x0:x1]
        mask = ~np.isclose(a, b, rtol=params.comparison_tolerance, atol=0.0, equal_nan=True)
        n = int(mask.sum())
        if n:
            if verbose:
                if not different:
                    print(f"At {label}:")
                print(f"  {n} differences found in {v}")
                for (j, i) in np.argwhere(mask)[:20]:
                    print(f"   - ({i + x0 - params.nghost + 1:3d},{j + y0 - params.nghost + 1:3d}): "
                          f"{a[j, i]:12.5g} ≢ {b[j, i]:12.5g} ({a[j, i] - b[j, i]:12.5g})")
            different = True
    return different


def step_checkpoint(params, grid, step_label, axis_letter):
    """ref src/io.jl:185-227: dump (is_ref) or diff (compare) the state after one sub-step. Returns True when
    a difference was found (the caller stops the cycle, like the reference's ``@checkpoint``)."""
    if not params.compare:
        return False
    gdt = grid.global_dt
    name = f"{params.output_file}_{gdt.cycle:03d}_{step_label}_{axis_letter}"
    if params.is_ref:
        if step_label == "time_step":
            write_time_step_file(params, gdt.current_dt, name)
        else:
            write_sub_domain_file(params, grid, name, no_msg=True)
        return False
    if step_label == "time_step":
        ref_dt = read_time_step_file(params, name)
        different = not np.isclose(ref_dt, gdt.current_dt, rtol=params.comparison_tolerance, atol=0.0)
        if different:
            print(f"Time step difference: ref Δt = {ref_dt:.18f}, Δt = {gdt.current_dt:.18f}, "
                  f"diff = {ref_dt - gdt.current_dt:.18f}")
    else:
        ref = read_sub_domain_file(params, name)
        different = compare_host(params, ref, grid.device_to_host(SAVED_VARS), step_label)
    if params.use_MPI:
        from .halo_exchange import allreduce_sum
        different = allreduce_sum(params, (float(different),))[0] > 0
    if different:
        write_sub_domain_file(params, grid, name + "_diff", no_msg=True)
        print(f"Difference file written to {name}_diff")
    return different


PROFILE_COLUMNS = ("coord", "n", "rho", "un", "ut", "E", "p", "rho_min", "rho_max", "p_min", "p_max")


def write_profile_file(path, profile, precision=17):
    """A profile (profile.Profile) as text: a header line — kind, centre and dr (r) or width (x, y), cycle, time — then one
    line per bin: coordinate, n, the five means, the four extrema, at ``precision`` digits (17 reads back bit for bit)."""
    t = profile.table()
    fmt = _fmt(precision)
    head = [f"# profile kind={t['kind']}"]
    if t["kind"] == "r":
        head += [f"centre_x={fmt % t['centre'][0]}", f"centre_y={fmt % t['centre'][1]}", f"dr={fmt % t['dr']}"]
    else:
        head.append(f"width={t['width']}")
    head += [f"cycle={t['cycle']}", f"time={fmt % t['time']}"]
    with open(path, "w") as f:
        f.write(" ".join(h.replace("= ", "=") for h in head) + "\n")
        f.write("# " + ", ".join(PROFILE_COLUMNS) + "\n")
        for b in range(len(t["n"])):
            f.write(", ".join(str(int(t[c][b])) if c == "n" else fmt % t[c][b] for c in PROFILE_COLUMNS) + "\n")


def read_profile_file(path):
    """→ the dict of ``Profile.table()``: kind, cycle, time, centre and dr or width, and one fp64 array per column (``n``: uint64)."""
    with open(path) as f:
        head = dict(item.split("=", 1) for item in f.readline().split()[2:])
        f.readline()
        rows = [[v.strip() for v in line.split(",")] for line in f if line.strip()]
    t = {"kind": head["kind"], "cycle": int(head["cycle"]), "time": float(head["time"])}
    if t["kind"] == "r":
        t["centre"], t["dr"] = (float(head["centre_x"]), float(head["centre_y"])), float(head["dr"])
    else:
        t["width"] = int(head["width"])
    for k, c in enumerate(PROFILE_COLUMNS):
        t[c] = np.array([int(r[k]) for r in rows], dtype=np.uint64) if c == "n" else np.array([float(r[k]) for r in rows], dtype=np.float64)
    return t


MIXING_COLUMNS = ("coord", "n", "rho", "phi", "phi_favre", "variance", "favre_variance", "phi_min", "phi_max")
MIXING_MEASURES = ("content", "min", "max", "width", "mixedness", "extent_lo", "extent_hi")


def write_mixing_file(path, profiles, pdfs=None, precision=17):
    """One mixing sample (dict name → mixing.MixingProfile, dict name → mixing.ScalarPDF or None) as text: a header line —
    cycle, time, how many scalars and histograms — then per scalar a block of profile columns (a line naming the scalar, the
    axis, the width and the bins; a line naming the columns; one line per bin), and below them per histogram a block of
    ``edge_lo, edge_hi, count, mass`` (a line naming the scalar, the range, the bins, the bad count and what fell below and
    above; one line per bin), at ``precision`` digits (17 reads back bit for bit)."""
    fmt = _fmt(precision)
    tables = [p.table() for p in profiles.values()]
    with open(path, "w") as f:
        f.write(f"# mixing cycle={tables[0]['cycle']} time={(fmt % tables[0]['time']).strip()} scalars={len(tables)} "
                f"pdfs={len(pdfs or {})}\n")
        for t in tables:
            f.write(f"# scalar name={t['name']} axis={t['axis']} width={t['width']} nbins={len(t['n'])}\n")
            f.write("# " + ", ".join(MIXING_COLUMNS) + "\n")
            for b in range(len(t["n"])):
                f.write(", ".join(str(int(t[c][b])) if c == "n" else fmt % t[c][b] for c in MIXING_COLUMNS) + "\n")
        for pdf in (pdfs or {}).values():
            t = pdf.table()
            f.write(f"# pdf name={t['name']} lo={(fmt % t['lo']).strip()} hi={(fmt % t['hi']).strip()} nbins={t['nbins']} bad={t['bad']} "
                    f"below_n={t['below'][0]} below_mass={(fmt % t['below'][1]).strip()} above_n={t['above'][0]} "
                    f"above_mass={(fmt % t['above'][1]).strip()}\n")
            f.write("# edge_lo, edge_hi, count, mass\n")
            for b in range(t["nbins"]):
                f.write(f"{fmt % t['edges'][b]}, {fmt % t['edges'][b + 1]}, {int(t['counts'][b])}, {fmt % t['mass'][b]}\n")


def read_mixing_file(path):
    """→ ``(profiles, pdfs)``: dict name → the dict of ``MixingProfile.table()``, and dict name → the dict of
    ``ScalarPDF.table()`` or None when the file holds no histogram."""
    with open(path) as f:
        lines = [line.rstrip("\n") for line in f if line.strip()]
    head = dict(item.split("=", 1) for item in lines[0].split()[2:])
    cycle, time = int(head["cycle"]), float(head["time"])
    profiles, pdfs, at = {}, {}, 1
    for _ in range(int(head["scalars"])):
        h = dict(item.split("=", 1) for item in lines[at].split()[2:])
        nb = int(h["nbins"])
        rows = [[v.strip() for v in line.split(",")] for line in lines[at + 2:at + 2 + nb]]
        t = {"name": h["name"], "axis": h["axis"], "width": int(h["width"]), "cycle": cycle, "time": time}
        for k, c in enumerate(MIXING_COLUMNS):
            t[c] = np.array([int(r[k]) for r in rows], dtype=np.uint64) if c == "n" else np.array([float(r[k]) for r in rows], dtype=np.float64)
        profiles[t["name"]] = t
        at += 2 + nb
    for _ in range(int(head["pdfs"])):
        h = dict(item.split("=", 1) for item in lines[at].split()[2:])
        nb = int(h["nbins"])
        rows = [[v.strip() for v in line.split(",")] for line in lines[at + 2:at + 2 + nb]]
        edges = [float(r[0]) for r in rows] + [float(rows[-1][1])]
        pdfs[h["name"]] = {"name": h["name"], "lo": float(h["lo"]), "hi": float(h["hi"]), "nbins": nb, "bad": int(h["bad"]),
                           "below": (int(h["below_n"]), float(h["below_mass"])), "above": (int(h["above_n"]), float(h["above_mass"])),
                           "edges": np.array(edges, dtype=np.float64), "counts": np.array([int(r[2]) for r in rows], dtype=np.uint64),
                           "mass": np.array([float(r[3]) for r in rows], dtype=np.float64)}
        at += 2 + nb
    return profiles, (pdfs or None)


def write_mixing_series(path, samples, precision=17):
    """The time series of a run's mixing samples ``(cycle, time, profiles, pdfs)`` as text: a header line naming the scalars,
    a line naming the columns, then one line per sample: cycle, time, and per scalar the content, the minimum, the maximum,
    the integral width W, the mixedness Θ and both ends of ``extent()`` (NaN where there is none)."""
    fmt = _fmt(precision)
    names = list(samples[0][2]) if samples else []
    with open(path, "w") as f:
        f.write("# mixing_series scalars=" + ",".join(names) + "\n")
        f.write("# cycle, time" + "".join(f", {s}:{m}" for s in names for m in MIXING_MEASURES) + "\n")
        for cycle, time, profiles, _ in samples:
            values = [profiles[s].measures()[m] for s in names for m in MIXING_MEASURES]
            f.write(", ".join([str(int(cycle)), fmt % time] + [fmt % v for v in values]) + "\n")


def read_mixing_series(path):
    """→ dict: ``scalars`` (names), ``cycle`` (int64 array), ``time`` (fp64 array) and per scalar name a dict measure → fp64
    array, the measures being ``MIXING_MEASURES``."""
    with open(path) as f:
        head = f.readline().split()[2]
        f.readline()
        rows = [[v.strip() for v in line.split(",")] for line in f if line.strip()]
    names = [s for s in head.split("=", 1)[1].split(",") if s]
    t = {"scalars": names, "cycle": np.array([int(r[0]) for r in rows], dtype=np.int64),
         "time": np.array([float(r[1]) for r in rows], dtype=np.float64)}
    for i, s in enumerate(names):
        t[s] = {m: np.array([float(r[2 + i * len(MIXING_MEASURES) + k]) for r in rows], dtype=np.float64)
                for k, m in enumerate(MIXING_MEASURES)}
    return t


ERROR_NORMS_COLUMNS = ("l1", "l2", "linf", "bias")


def write_error_norms_file(path, norms, precision=17):
    """Error norms (analytic.ErrorNorms) as text: a header line — cycle, time, samples, n, n_bad — then one line per variable
    (rho, un, ut, p): L1, L2, Linf, bias at ``precision`` digits (17 reads back bit for bit) and the global cell (gx, gy) that
    attains Linf, -1 -1 when no cell differs."""
    t = norms.table()
    fmt = _fmt(precision)
    with open(path, "w") as f:
        f.write(f"# error_norms cycle={t['cycle']} time={(fmt % t['time']).strip()} samples={t['samples']} n={t['n']} n_bad={t['n_bad']}\n")
        f.write("# variable, " + ", ".join(ERROR_NORMS_COLUMNS) + ", linf_gx, linf_gy\n")
        for name in ("rho", "un", "ut", "p"):
            at = t[name]["linf_at"] or (-1, -1)
            f.write(", ".join([name] + [fmt % t[name][c] for c in ERROR_NORMS_COLUMNS] + [str(at[0]), str(at[1])]) + "\n")


def read_error_norms_file(path):
    """→ the dict of ``ErrorNorms.table()``."""
    with open(path) as f:
        head = dict(item.split("=", 1) for item in f.readline().split()[2:])
        f.readline()
        rows = [[v.strip() for v in line.split(",")] for line in f if line.strip()]
    t = {"cycle": int(head["cycle"]), "time": float(head["time"]), "samples": int(head["samples"]), "n": int(head["n"]),
         "n_bad": int(head["n_bad"])}
    for r in rows:
        at = (int(r[5]), int(r[6]))
        t[r[0]] = {c: float(r[1 + k]) for k, c in enumerate(ERROR_NORMS_COLUMNS)}
        t[r[0]]["linf_at"] = None if at == (-1, -1) else at
    return t


# ---- run history (history.py): one text file per run, a row per sample --------------------------------------------------
HISTORY_FMT = "%#24.17e"


def _history_header(history, global_grid):
    """The ``#`` lines of a history file: the format version, the global grid, the six scale exponents, ``ds``, every gauge
    point with its cell, and the column names."""
    from .history import COLUMNS, FORMAT_VERSION, GAUGE_VARS
    lines = [f"# history version={FORMAT_VERSION}",
             f"# N={int(global_grid[0])},{int(global_grid[1])}",
             "# scale_exp=" + ",".join(str(s) for s in history.scale_exp),
             f"# ds={float(history.ds).hex()}"]
    for i, ((x, y), (gx, gy)) in enumerate(zip(history.gauges, history.gauge_cells)):
        lines.append(f"# gauge{i}={float(x).hex()},{float(y).hex()},{gx},{gy}")
    columns = list(COLUMNS) + [f"g{i}_{name}" for i in range(len(history.gauges)) for name in GAUGE_VARS]
    lines.append("# columns=" + ",".join(columns))
    return lines


def write_history_file(path, history, global_grid):
    """A history (history.History) as text: the header (``_history_header``), then one row per sample, every column as
    ``%#24.17e`` (reads back bit for bit). Replaces the file."""
    with open(path, "w") as f:
        f.write("\n".join(_history_header(history, global_grid)) + "\n")
    append_history_rows(path, history, 0)


def append_history_rows(path, history, start):
    """Rows ``start`` … of ``history`` appended to its file."""
    rows = history.rows(start)
    if rows:
        with open(path, "a") as f:
            for row in rows:
                f.write(" ".join(HISTORY_FMT % v for v in row) + "\n")


def read_history_header(path):
    """The header fields of a history file → dict field → text, ``scale_exp`` as a tuple of ints."""
    head = {}
    with open(path) as f:
        for line in f:
            if not line.startswith("#"):
                break
            item = line[1:].strip()
            if item.startswith("history "):
                item = item[len("history "):]
            key, _, value = item.partition("=")
            head[key.strip()] = value.strip()
    for field in ("version", "N", "scale_exp", "ds", "columns"):
        if field not in head:
            from ._lib import solver_error
            solver_error("config", f"{path} is not a history file: its header has no {field}")
    head["scale_exp"] = tuple(int(s) for s in head["scale_exp"].split(","))
    return head


def check_history_header(path, head, history, global_grid):
    """A restart appends to the file of the run it continues only when the header is the one this run would write: a
    configuration error that names the first field that differs."""
    from ._lib import solver_error
    want = read_history_header_lines(_history_header(history, global_grid))
    fields = [k for k in head if k != "columns"] + [k for k in want if k not in head and k != "columns"] + ["columns"]
    for field in fields:                        # (the columns last: they follow from the gauges)
        if head.get(field) != want.get(field):
            solver_error("config", f"{path} does not continue as this run's history: {field} is {head.get(field)!r} in the file, "
                                   f"{want.get(field)!r} for this run")


def read_history_header_lines(lines):
    head = {}
    for line in lines:
        item = line[1:].strip()
        if item.startswith("history "):
            item = item[len("history "):]
        key, _, value = item.partition("=")
        head[key.strip()] = value.strip()
    head["scale_exp"] = tuple(int(s) for s in head["scale_exp"].split(","))
    return head


def truncate_history_file(path, cycle):
    """Keep the header and the rows up to and including ``cycle``; later rows are dropped."""
    with open(path) as f:
        lines = f.readlines()
    keep = [line for line in lines if line.startswith("#") or (line.strip() and float(line.split()[0]) <= cycle)]
    with open(path, "w") as f:
        f.writelines(keep)


def read_history_file(path):
    """→ the dict of ``History.table()``: version, scale_exp, ds, global_nx, gauges, gauge_cells and one fp64 array per column."""
    head = read_history_header(path)
    gauges, cells, i = [], [], 0
    while f"gauge{i}" in head:
        x, y, gx, gy = head[f"gauge{i}"].split(",")
        gauges.append((float.fromhex(x), float.fromhex(y)))
        cells.append((int(gx), int(gy)))
        i += 1
    columns = head["columns"].split(",")
    with open(path) as f:
        rows = [[float(v) for v in line.split()] for line in f if line.strip() and not line.startswith("#")]
    data = np.array(rows, dtype=np.float64).reshape(len(rows), len(columns))
    t = {"version": int(head["version"]), "scale_exp": head["scale_exp"], "ds": float.fromhex(head["ds"]),
         "global_nx": int(head["N"].split(",")[0]), "gauges": tuple(gauges), "gauge_cells": tuple(cells)}
    for k, c in enumerate(columns):
        t[c] = data[:, k].copy()
    return t


# ---- in-situ images (derived.py) -------------------------------------------------------------------------------------------
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind, payload):
    import struct
    import zlib
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xffffffff)


def write_png_gray8(path, img):
    """An 8-bit greyscale PNG of the ``(height, width)`` uint8 array ``img`` (row 0 = the top row of the picture), written with
    the standard library only: IHDR, one IDAT of the zlib-compressed rows (each behind a filter byte 0), IEND."""
    import struct
    import zlib
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"write_png_gray8 takes a non-empty (height, width) uint8 array, got {img.dtype} {img.shape}")
    h, w = img.shape
    rows = np.zeros((h, w + 1), dtype=np.uint8)         # filter type 0 (None) in front of every row
    rows[:, 1:] = img
    with open(path, "wb") as f:
        f.write(PNG_SIGNATURE)
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)))
        f.write(_png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(_png_chunk(b"IEND", b""))
    return path


def read_png_chunks(path):
    """``[(kind, payload, crc_ok)]`` of every chunk of a PNG file (the signature is checked)."""
    import struct
    import zlib
    data = open(path, "rb").read()
    if data[:8] != PNG_SIGNATURE:
        raise ValueError(f"{path} is not a PNG file")
    chunks, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        chunks.append((kind, payload, crc == (zlib.crc32(kind + payload) & 0xffffffff)))
        at += 12 + n
    return chunks


def read_png_gray8(path):
    """What ``write_png_gray8`` wrote → the ``(height, width)`` uint8 array. Only 8-bit greyscale, no interlace, filter 0."""
    import struct
    import zlib
    chunks = read_png_chunks(path)
    if not chunks or chunks[0][0] != b"IHDR" or chunks[-1][0] != b"IEND" or not all(ok for _, _, ok in chunks):
        raise ValueError(f"{path}: a damaged PNG file (chunk order or CRC)")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if (depth, colour, comp, filt, lace) != (8, 0, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit greyscale PNG files without interlace are read")
    raw = zlib.decompress(b"".join(p for k, p, _ in chunks if k == b"IDAT"))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, w + 1)
    if rows[:, 0].any():
        raise ValueError(f"{path}: only rows of filter type 0 are read")
    return rows[:, 1:].copy()
