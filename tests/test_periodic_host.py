"""Periodic sides on the host (no GPU): the third boundary type of a ``Problem``, how it sets the run's
``periodic``, digests and checkpoint headers, the exact solutions that no longer apply, and the new entry point's binding."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

import armon_amd
from armon_amd import ArmonParameters, HalfPlane, Problem, SolverException, State, checkpoint
from armon_amd.blocking import Side
from armon_amd.parameters import PROC_NULL, resolve_periodic
from armon_amd.boundaries import periodic_axes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, F, P = "Dirichlet", "FreeFlow", "Periodic"


def config_error(call):
    with pytest.raises(SolverException) as e:
        call()
    assert e.value.category == "config", e.value
    return e.value.msg


def box(**kw):
    return Problem("box", State(1., p=1.), [(HalfPlane((1, 0), 0.5), State(2., p=2.))], **kw)


# ---- the boundary type -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,axes", [((P, P, W, W), (True, False)), ((F, W, P, P), (False, True)),
                                    ((P, P, P, P), (True, True)), (W, (False, False)), ((W, F, F, W), (False, False))])
def test_periodic_is_a_boundary_type_and_sets_the_runs_periodic(b, axes):
    prob = box(boundaries=b)
    assert periodic_axes(prob.boundaries) == axes
    params = ArmonParameters(test=prob, N=(16, 12))
    assert params.periodic == axes and params.wrap == axes
    assert all(n == PROC_NULL for n in params.neighbours.values())      # a lone block: the process grid does not wrap
    assert params.test.boundaries == prob.boundaries
    if axes == (True, True):
        assert all(params.test.boundary_condition(s) == (1., 1.) for s in Side)     # the neutral pair: no mirror


def test_like_takes_boundaries():
    sedov = Problem.like("Sedov", boundaries=P)
    assert sedov.boundaries == (P,) * 4 and ArmonParameters(test=sedov, N=(16, 16)).periodic == (True, True)
    assert Problem.like("Sod", boundaries=(W, W, P, P)).boundaries == (W, W, P, P)
    assert Problem.like("Sod").boundaries == (W, W, F, F)
    rho = np.ones((12, 16))
    arrays = Problem.from_arrays(rho, 0 * rho, 0 * rho, p=rho, boundaries=P)
    assert ArmonParameters(test=arrays, N=(16, 12)).wrap == (True, True)


@pytest.mark.parametrize("b", ["periodic", "Wall", ("Periodic",) * 3, ("Periodic", "Periodic", "Dirichlet", "wrap"), 3, None])
def test_a_bad_boundaries_value_names_the_three_types(b):
    makes = [lambda: box(boundaries=b)] + ([lambda: Problem.like("Sod", boundaries=b)] if b is not None else [])   # (None: the case's own)
    for make in makes:
        msg = config_error(make)
        assert "boundaries" in msg and all(f"'{t}'" in msg for t in (W, F, P)), msg


def test_the_constructors_one_word_shorthand_is_what_it_was():
    """``Problem(boundaries=word)`` keeps its two words; periodic sides are named side by side there, and the refusal says so.
    The presets spell the one word out for the four sides."""
    assert box(boundaries=W).boundaries == (W,) * 4 and box(boundaries=F).boundaries == (F,) * 4
    msg = config_error(lambda: box(boundaries=P))
    assert "boundaries" in msg and "side by side" in msg and all(f"'{t}'" in msg for t in (W, F, P)), msg
    assert box(boundaries=(P,) * 4).boundaries == (P,) * 4
    left, right = State(1., p=1.), State(0.125, p=0.1)
    assert Problem.riemann(left, right, boundaries=P).boundaries == (P,) * 4
    assert Problem.four_quadrants([left, right, left, right], boundaries=P).boundaries == (P,) * 4
    assert Problem.four_quadrants([left, right, left, right]).boundaries == (F,) * 4


@pytest.mark.parametrize("b,axis", [((P, W, F, F), "x"), ((W, P, F, F), "x"), ((F, F, P, W), "y"), ((P, P, F, P), "y"),
                                    ((F, P, P, P), "x")])
def test_one_sided_periodicity_is_refused_and_names_the_axis(b, axis):
    for make in (lambda: box(boundaries=b), lambda: Problem.like("Sod_circ", boundaries=b)):
        msg = config_error(make)
        assert f"the {axis} axis" in msg and "periodic together" in msg, msg


def test_a_problem_and_the_option_must_agree():
    px = box(boundaries=(P, P, W, W))
    assert ArmonParameters(test=px, N=(16, 12), periodic=(True, False)).periodic == (True, False)
    for bad in ((False, False), (True, True), (False, True)):
        msg = config_error(lambda: ArmonParameters(test=px, N=(16, 12), periodic=bad))
        assert "contradicts" in msg and "periodic" in msg, msg
        msg = config_error(lambda: resolve_periodic(px, bad))
        assert "contradicts" in msg
    # a test without periodic sides of its own: the option overrides its sides on that axis, as it does in groups
    for test in ("Sod_circ", box()):
        params = ArmonParameters(test=test, N=(16, 12), periodic=(False, True))
        assert params.periodic == params.wrap == (False, True)
        tile = ArmonParameters(test=test, N=(16, 12), periodic=(False, True), tile_of=(0, (1, 2)))
        assert tile.periodic == (False, True) and tile.wrap == (False, False)
        assert tile.neighbours[Side.Bottom] == 1 and tile.neighbours[Side.Top] == 1 and tile.neighbours[Side.Left] == PROC_NULL
    for bad in (True, (True,), (1, 2), ("yes", "no"), (None, None)):
        msg = config_error(lambda: ArmonParameters(test="Sod", N=(16, 12), periodic=bad))
        assert "two booleans" in msg, msg


def test_a_tile_of_a_periodic_problem_wraps_its_topology():
    prob = box(boundaries=(P, P, W, W))
    tile = ArmonParameters(test=prob, N=(16, 12), tile_of=(1, (2, 1)))
    assert tile.periodic == (True, False) and tile.wrap == (False, False)
    assert tile.neighbours[Side.Left] == 0 and tile.neighbours[Side.Right] == 0
    assert tile.neighbours[Side.Bottom] == PROC_NULL and tile.neighbours[Side.Top] == PROC_NULL


def test_the_lone_blocks_sweeps_read_the_ghosts_of_a_periodic_axis():
    """``sweep_desc`` needs a grid (a device); what it decides from is ``wrap``: stated here on the parameters, the GPU tests run
    it. The pair path is kept for X, not for Y; graph replay falls back."""
    from armon_amd.solver import graph_cycles_usable, pair_usable
    kw = dict(test="Sod_circ", N=(64, 64), placement_min_bytes=1, silent=5)
    assert pair_usable(ArmonParameters(**kw)) and pair_usable(ArmonParameters(periodic=(True, False), **kw))
    assert not pair_usable(ArmonParameters(periodic=(False, True), **kw))
    assert not pair_usable(ArmonParameters(periodic=(True, True), **kw))
    for per in ((True, False), (False, True), (True, True)):
        assert not graph_cycles_usable(ArmonParameters(graph_cycles=True, periodic=per, **kw))


# ---- digests -----------------------------------------------------------------------------------------------------------------
# sha256 of the canonical description of the presets at N = (16, 12), fp64, recorded from the parent commit
PARENT_KEYS = ("arrays", "background", "boundaries", "eos", "gamma", "regions", "samples")


def canonical(test):
    return hashlib.sha256(json.dumps({k: test.description[k] for k in PARENT_KEYS}, sort_keys=True).encode("utf-8")).hexdigest()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["Sod", "Sod_y", "Sod_circ", "Bizarrium", "Sedov"])
def test_the_digests_of_the_presets_do_not_move(name, dtype):
    """The description of a problem without periodic sides holds exactly the seven keys it held, with the same values: its
    digest, recomputed from them, is the stored one — and it does not depend on whether ``periodic`` was spelled out."""
    kw = dict(N=(16, 12), data_type=dtype)
    a = ArmonParameters(test=Problem.like(name), **kw).test
    b = ArmonParameters(test=Problem.like(name), periodic=(False, False), **kw).test
    assert sorted(a.description) == sorted(PARENT_KEYS)
    assert a.digest == b.digest == canonical(a)
    assert a.description["boundaries"] == list(armon_amd.test_cases._known(name)["boundaries"])


def test_a_periodic_problems_digest_differs_through_boundaries_only():
    kw = dict(N=(16, 12))
    wall, wrapped = ArmonParameters(test=box(), **kw).test, ArmonParameters(test=box(boundaries=(P, P, W, W)), **kw).test
    assert wall.digest != wrapped.digest
    assert sorted(wrapped.description) == sorted(PARENT_KEYS)
    assert {k for k in PARENT_KEYS if wall.description[k] != wrapped.description[k]} == {"boundaries"}
    assert wrapped.description["boundaries"] == [P, P, W, W]


# ---- the exact solutions -----------------------------------------------------------------------------------------------------
def test_no_closed_form_across_a_periodic_axis():
    from armon_amd import analytic as an
    left, right = State(1., p=1.), State(0.125, p=0.1)
    for axis, along, across in (("x", (P, P, F, F), (W, W, P, P)), ("y", (F, F, P, P), (P, P, W, W))):
        ok = ArmonParameters(test=Problem.riemann(left, right, axis=axis, boundaries=across), N=(32, 8))
        assert an.has_closed_form(ok.test, ok.periodic) and an.reference_for(ok, 0.1) is not None
        bad = ArmonParameters(test=Problem.riemann(left, right, axis=axis, boundaries=along), N=(32, 8))
        assert not an.has_closed_form(bad.test) and not an.has_closed_form(bad.test, bad.periodic)
        with pytest.raises(SolverException) as e:
            an.reference_for(bad, 0.1)
        assert e.value.category == "analytic" and "no closed-form" in e.value.msg
        msg = config_error(lambda: ArmonParameters(test=Problem.riemann(left, right, axis=axis, boundaries=along), N=(32, 8),
                                                   error_norms_at_end=True))
        assert "no closed form" in msg
    # a built-in case whose axis the option makes periodic
    sod_y = ArmonParameters(test="Sod", N=(32, 8), periodic=(False, True))
    assert an.reference_for(sod_y, 0.1) is not None
    with pytest.raises(SolverException, match="no closed-form"):
        an.reference_for(ArmonParameters(test="Sod", N=(32, 8), periodic=(True, False)), 0.1)
    with pytest.raises(SolverException, match="no closed-form"):
        an.reference_for(ArmonParameters(test="Sod_y", N=(8, 32), periodic=(False, True)), 0.1)


def test_a_periodic_problem_stays_conservative():
    assert ArmonParameters(test=box(boundaries=(P,) * 4), N=(16, 12)).test.conservative
    assert ArmonParameters(test="Sod_circ", N=(16, 12), periodic=(True, True)).test.conservative
    assert not ArmonParameters(test=box(boundaries=(P, P, W, W)), N=(16, 12), gravity=(0., -1.)).test.conservative


# ---- checkpoint headers ------------------------------------------------------------------------------------------------------
def header_of(params):
    h = dict(checkpoint.bit_options(params))
    h.update(cycle=3, time=float(0.01).hex())
    return h


def test_headers_periodic_against_plain_in_both_directions():
    kw = dict(N=(16, 12), maxcycle=10)
    for make in (lambda **o: ArmonParameters(test="Sod_circ", **kw, **o),
                 lambda periodic=None, **o: ArmonParameters(test=box(boundaries=(P, P, W, W) if periodic else W), **kw, **o)):
        plain, lone = make(), make(periodic=(True, False))
        tile = make(periodic=(True, False), tile_of=(0, (2, 1)))
        assert checkpoint.bit_options(lone)["periodic"] == [True, False]
        # a lone periodic block and a tile of a periodic group write, and take, the same header
        assert checkpoint.bit_options(lone) == checkpoint.bit_options(tile)
        checkpoint.check_compatible(lone, header_of(tile), "f.ckpt")
        checkpoint.check_compatible(tile, header_of(lone), "f.ckpt")
        for run, file in ((lone, plain), (plain, lone), (tile, plain), (plain, tile)):
            msg = config_error(lambda: checkpoint.check_compatible(run, header_of(file), "f.ckpt"))
            assert "periodic" in msg or "problem_digest" in msg, msg
    a, b = ArmonParameters(test="Sod_circ", periodic=(True, False), **kw), ArmonParameters(test="Sod_circ", periodic=(False, True), **kw)
    assert "periodic" in config_error(lambda: checkpoint.check_compatible(a, header_of(b), "f.ckpt"))


# ---- the entry point ---------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_exported_and_bound_as_the_header_declares():
    from armon_amd._lib import ALT_LIB_PATH, SIGNATURES
    text = open(os.path.join(ROOT, "include", "armon_hip.h")).read()
    C = ctypes
    ctype = {"armon_ctx*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "double* const*": C.POINTER(C.c_void_p),
             "float* const*": C.POINTER(C.c_void_p)}
    for name in ("armon_hip_periodic_ghosts", "armon_hip_periodic_ghosts_f32"):
        m = re.search(r"ARMON_API\s+int\s+" + name + r"\s*\(([^;]*?)\)\s*;", text)
        assert m, f"{name} is not declared in include/armon_hip.h"
        args = [re.sub(r"/\*.*?\*/", "", a, flags=re.S).strip() for a in m.group(1).split(",")]
        types = [a if a.endswith("*") else a.rsplit(" ", 1)[0].strip() for a in args]      # drop the parameter's name
        res, argtypes = SIGNATURES[name]
        assert res is C.c_int and argtypes == [ctype[t] for t in types], (name, types)
        for path in (armon_amd.LIB_PATH, ALT_LIB_PATH):
            assert hasattr(C.CDLL(path), name), f"{name} is not exported by {path}"
    assert "The rule, word for word" in text[text.index("Periodic sides (csrc/periodic.hip"):text.index("armon_hip_periodic_ghosts(")]


def test_refusals_that_need_no_device():
    """A NULL context is refused before anything is launched (the GPU tests go through the other refusals with a real one)."""
    L = armon_amd.lib()
    vars_ = (ctypes.c_void_p * 1)(8)
    assert L.armon_hip_periodic_ghosts(None, 0, 24, 4, 4, 16, 16, 1, vars_) != 0
    assert b"ctx" in L.armon_hip_last_error()
    assert L.armon_hip_periodic_ghosts_f32(None, 1, 24, 4, 4, 16, 16, 1, vars_) != 0
