"""In-situ reduced output, the parts that need no GPU: option validation, coarse shapes, the coarse file format."""
import numpy as np
import pytest

import armon_amd
from armon_amd import io
from armon_amd.parameters import ArmonParameters, coarse_shape, normalize_coarsen_factor


def test_output_coarsen_defaults_to_the_full_grid():
    assert ArmonParameters(test="Sod", N=(8, 8)).output_coarsen is None
    assert ArmonParameters(test="Sod", N=(8, 8), output_coarsen=0).output_coarsen is None
    assert ArmonParameters(test="Sod", N=(8, 8), output_coarsen=4).output_coarsen == (4, 4)
    assert ArmonParameters(test="Sod", N=(8, 8), output_coarsen=(8, 3)).output_coarsen == (8, 3)
    assert ArmonParameters(test="Sod", N=(8, 8), output_coarsen=np.int64(2)).output_coarsen == (2, 2)
    assert ArmonParameters(test="Sod", N=(8, 8), output_coarsen=[1, 100]).output_coarsen == (1, 100)   # larger than the grid


@pytest.mark.parametrize("factor", [-1, (4, 0), (0, 4), (0, 0), (-2, 2), 2.0, 2.5, (4, 1.5), "4", (4,), (1, 2, 3), True, None])
def test_invalid_factors_are_configuration_errors(factor):
    with pytest.raises(armon_amd.SolverException) as e:
        ArmonParameters(test="Sod", N=(64, 64), output_coarsen=factor)
    assert e.value.category == "config"
    with pytest.raises(armon_amd.SolverException) as e:
        normalize_coarsen_factor(factor)
    assert e.value.category == "config"


def test_coarsening_with_ghost_output_is_refused():
    with pytest.raises(armon_amd.SolverException) as e:
        ArmonParameters(test="Sod", N=(64, 64), output_coarsen=4, write_ghosts=True)
    assert e.value.category == "config" and "write_ghosts" in e.value.msg
    ArmonParameters(test="Sod", N=(64, 64), output_coarsen=0, write_ghosts=True)       # the default is untouched


def test_factor_must_respect_the_tile_boundaries():
    # 2x2 tiles of 64x48: tiles start at 0 / 32 along x and 0 / 24 along y
    for rank in range(4):
        p = ArmonParameters(test="Sod", N=(64, 48), tile_of=(rank, (2, 2)), output_coarsen=(16, 8))
        assert p.output_coarsen == (16, 8)
    with pytest.raises(armon_amd.SolverException) as e:
        ArmonParameters(test="Sod", N=(64, 48), tile_of=(1, (2, 2)), output_coarsen=(16, 16))     # 24 % 16 != 0
    assert e.value.category == "config" and "tile boundaries" in e.value.msg
    with pytest.raises(armon_amd.SolverException) as e:
        ArmonParameters(test="Sod", N=(64, 48), tile_of=(2, (2, 2)), output_coarsen=(5, 8))       # 32 % 5 != 0
    assert e.value.category == "config" and "tile boundaries" in e.value.msg
    # the first tile starts at 0: every factor is aligned there
    ArmonParameters(test="Sod", N=(64, 48), tile_of=(0, (2, 2)), output_coarsen=(5, 7))


@pytest.mark.parametrize("N,factor,shape", [
    ((1024, 1024), (16, 16), (64, 64)),
    ((1000, 777), (16, 16), (63, 49)),
    ((1000, 777), (7, 3), (143, 259)),
    ((1000, 777), (64, 8), (16, 98)),
    ((1000, 777), (1, 1), (1000, 777)),
    ((1000, 777), (2048, 4096), (1, 1)),
    ((5, 9), (5, 10), (1, 1)),
])
def test_coarse_shape_is_the_ceiling(N, factor, shape):
    assert coarse_shape(N, factor) == shape


def synthetic_planes(cnx, cny, dtype):
    rng = np.random.default_rng(cnx * 1000 + cny)
    planes = {k: rng.standard_normal((cny, cnx)).astype(dtype) for k in ("rho", "u", "v", "p", "E")}
    planes["x"] = np.broadcast_to(np.linspace(0, 1, cnx, endpoint=False, dtype=dtype)[None, :], (cny, cnx)).copy()
    planes["y"] = np.broadcast_to(np.linspace(0, 1, cny, endpoint=False, dtype=dtype)[:, None], (cny, cnx)).copy()
    return planes


@pytest.mark.parametrize("cnx,cny", [(7, 5), (1, 1), (1, 6), (9, 1)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_coarse_file_round_trip(tmp_path, cnx, cny, dtype):
    params = ArmonParameters(test="Sod", N=(64, 64), data_type=dtype, output_dir=str(tmp_path), output_coarsen=8)
    planes = synthetic_planes(cnx, cny, dtype)
    path = io.write_coarse_file(params, planes, "coarse")
    lines = open(path).read().split("\n")
    assert lines[-1] == ""                                           # the file ends with a newline
    lines = lines[:-1]
    assert sum(1 for l in lines if l.strip()) == cnx * cny           # one line per coarse cell
    assert len(lines) == cnx * cny + (cny - 1)                       # and one blank line between coarse rows
    for j in range(1, cny):
        assert lines[j * (cnx + 1) - 1] == ""
    # the reference's cell format: 6 fields "x, y, rho, u, v, p" of width precision + 7
    first = lines[0].split(", ")
    assert len(first) == 6 and all(len(t) == params.output_precision + 7 for t in first)
    back = io.read_coarse_file(params, "coarse")
    assert set(back) == set(io.SAVED_VARS)
    for k in io.SAVED_VARS:
        assert back[k].shape == (cny, cnx)
        # 17 significant digits carry a double (and a float) exactly
        assert np.array_equal(back[k], planes[k].astype(np.float64)), k


def test_coarse_file_reader_refuses_ragged_files(tmp_path):
    params = ArmonParameters(test="Sod", N=(64, 64), output_dir=str(tmp_path))
    with open(tmp_path / "bad", "w") as f:
        f.write("1, 2, 3, 4, 5, 6\n1, 2, 3, 4, 5, 6\n\n1, 2, 3, 4, 5, 6\n")
    with pytest.raises(ValueError):
        io.read_coarse_file(params, "bad")


def test_new_entry_points_are_bound_in_both_precisions():
    from armon_amd._lib import SIGNATURES
    for name in ("coarsen", "gather_strided"):
        for suffix in ("", "_f32"):
            assert "armon_hip_" + name + suffix in SIGNATURES
    L = armon_amd.lib()
    import ctypes as C
    # refused before anything touches a device: NULL context
    assert L.armon_hip_coarsen(None, 16, 4, 8, 8, 2, 2, None, None, None, None, None, None) == 1
    assert L.armon_hip_gather_strided(None, 10, 1, (C.c_void_p * 1)(), 0, 1, 1, None) == 1
