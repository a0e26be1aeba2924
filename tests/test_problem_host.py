"""User-defined problems on the host (no GPU): ``State``, the shapes, ``Problem`` and its presets, the canonical digest, and
the numpy restatement of the region rule (tests/regions_restated.py) on hand-worked cells."""
import math

import numpy as np
import pytest

from armon_amd import ArmonParameters, Box, Disc, Ellipse, HalfPlane, Problem, SolverException, State
from armon_amd.blocking import Side
from armon_amd import test_cases

import regions_restated as R


def test_a_state_derives_E_from_p_in_the_working_precision():
    s = State(0.7, u=0.3, v=-0.2, p=1.1)
    for T in (np.float64, np.float32):
        rho, u, v, p = T(0.7), T(0.3), T(-0.2), T(1.1)
        want = p / ((T(5 / 3) - T(1)) * rho) + (u * u + v * v) / T(2)
        got = s.energy(5 / 3, T)
        assert type(got) is T and got == want
        assert s.values(5 / 3, T) == (rho, u, v, want)
    # the two precisions do not agree, and neither is the other one rounded
    assert float(s.energy(5 / 3, np.float32)) != float(np.float32(s.energy(5 / 3, np.float64)))
    # why the presets pass E: the energy of p = 1 at rho = 1 is not 2.5
    assert float(State(1., p=1.).energy(7 / 5)) == 2.5000000000000004
    assert float(State(1., E=2.5).energy(7 / 5)) == 2.5


@pytest.mark.parametrize("kw", [dict(), dict(p=1., E=2.5)])
def test_a_state_with_both_or_neither_of_p_and_E_is_refused(kw):
    with pytest.raises(SolverException, match="exactly one of p and E"):
        State(1., **kw)


@pytest.mark.parametrize("kw", [dict(rho=0., p=1.), dict(rho=-1., E=1.), dict(rho=float("nan"), p=1.), dict(rho=1., u=float("inf"), p=1.)])
def test_a_state_that_is_not_finite_with_positive_density_is_refused(kw):
    with pytest.raises(SolverException):
        State(**kw)


def test_a_bizarrium_problem_with_a_state_given_by_p_is_refused():
    with pytest.raises(SolverException, match="bizarrium"):
        Problem("b", State(1e4, E=3e4), [(HalfPlane((1, 0), 0.5), State(1.4e4, p=1e9))], eos="bizarrium")
    with pytest.raises(SolverException, match="bizarrium"):
        Problem("b", State(1e4, p=3e4), eos="bizarrium")
    Problem("b", State(1e4, E=3e4), [(HalfPlane((1, 0), 0.5), State(1.4e4, E=4e6))], eos="bizarrium")


@pytest.mark.parametrize("b", ["Periodic", ("Dirichlet",) * 3, ("Dirichlet", "FreeFlow", "Dirichlet", "wall"), 3, None])
def test_a_bad_boundaries_value_is_refused(b):
    with pytest.raises(SolverException, match="boundaries"):
        Problem("p", State(1., p=1.), boundaries=b)


def test_boundaries_give_the_mirror_factors():
    p = ArmonParameters(test=Problem("p", State(1., p=1.), boundaries=("Dirichlet", "FreeFlow", "FreeFlow", "Dirichlet"))).test
    assert [p.boundary_condition(s) for s in (Side.Left, Side.Right, Side.Bottom, Side.Top)] == [(-1., 1.), (1., 1.), (1., 1.), (1., -1.)]
    q = ArmonParameters(test=Problem("p", State(1., p=1.), boundaries="FreeFlow")).test
    assert all(q.boundary_condition(s) == (1., 1.) for s in Side)


def test_more_than_32_regions_are_refused():
    regions = [(Disc((0.5, 0.5), r=0.01 * k), State(1., p=1.)) for k in range(1, 34)]
    Problem("p", State(1., p=1.), regions[:32])
    with pytest.raises(SolverException, match="33 regions"):
        Problem("p", State(1., p=1.), regions)


@pytest.mark.parametrize("samples", [0, 3, 16, True, 2.5])
def test_a_bad_sample_count_is_refused(samples):
    with pytest.raises(SolverException, match="samples"):
        Problem("p", State(1., p=1.), samples=samples)


def test_bad_shapes_are_refused():
    for make in (lambda: HalfPlane((0, 0), 1.), lambda: HalfPlane((1, float("nan")), 1.), lambda: Disc((0, 0)), lambda: Disc((0, 0), r=1., r2=1.),
                 lambda: Disc((float("inf"), 0), r=1.), lambda: Box(x=(float("nan"), 1.)), lambda: Ellipse((0, 0), (0., 1.)),
                 lambda: Problem("p", State(1., p=1.), [(HalfPlane((1, 0), 0.5), 3.0)])):
        with pytest.raises(SolverException):
            make()
    Box(x=(-math.inf, 0.5))                     # an open side is what an infinity in a box means


@pytest.mark.parametrize("name", ["Sod", "Sod_y", "Sod_circ", "Sedov", "Bizarrium"])
def test_a_preset_carries_the_settings_of_the_built_in_case(name):
    case = test_cases.TestCase(name=name, **test_cases._CASES[name])
    like = Problem.like(name)
    for key in ("boundaries", "cfl", "maxtime", "domain_size", "origin", "conservative", "eos"):
        assert getattr(like, key) == getattr(case, key), key
    a, b = ArmonParameters(test=name, N=(20, 30)), ArmonParameters(test=like, N=(20, 30))
    for key in ("domain_size", "origin", "cfl", "maxtime"):
        assert getattr(a, key) == getattr(b, key), key
    assert b.test.gamma == a.test.gamma == 7 / 5 and b.test.eos == a.test.eos and b.test.conservative == a.test.conservative
    assert all(b.test.boundary_condition(s) == a.test.boundary_condition(s) for s in Side)
    assert b.test.is_problem and b.test.header_name == "Problem:" + name
    # the options override a problem's values as they override a case's
    c = ArmonParameters(test=like, N=(20, 30), cfl=0.3, maxtime=0.01, domain_size=(2., 3.), origin=(-1., 0.5))
    assert (c.cfl, c.maxtime, c.domain_size, c.origin) == (0.3, 0.01, (2., 3.), (-1., 0.5))


def test_an_unknown_preset_is_refused():
    with pytest.raises(SolverException):
        Problem.like("DebugIndexes")
    with pytest.raises(SolverException):
        Problem.like("Noh")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_the_sedov_preset_follows_the_cell_size(dtype):
    """Its radius and inner energy are create_test's and init_test's, evaluated when the parameters know dX."""
    built_in = ArmonParameters(test="Sedov", N=(30, 50), data_type=dtype)
    T = built_in.T
    t = ArmonParameters(test=Problem.like("Sedov"), N=(30, 50), data_type=dtype).test
    (kind, a, state), = t.table
    r = T(built_in.test.r)
    assert kind == R.DISC and tuple(float(v) for v in a) == (0., 0., float(r * r), 0.)
    assert float(state[3]) == float(T(float((1 / 1.033) ** 5 / float(T(math.pi) * (r * r)))))
    other = ArmonParameters(test=Problem.like("Sedov"), N=(60, 50), data_type=dtype).test
    assert other.table[0][1][2] != a[2] and other.digest != t.digest


def implosion(**kw):
    return Problem("implosion", State(1., p=1.), [(HalfPlane((1, 1), 0.15), State(0.125, p=0.14))], domain_size=(0.3, 0.3),
                   samples=4, **kw)


def digest(problem, **kw):
    return ArmonParameters(test=problem, N=(16, 16), **kw).test.digest


def test_the_digest_is_stable_and_tells_problems_apart():
    a, b = digest(implosion()), digest(implosion())
    assert a == b and len(a) == 64 and int(a, 16) >= 0
    assert ArmonParameters(test=implosion(), N=(48, 48)).test.digest == a          # (no constant of it depends on the cell size)
    two = [(Disc((0.5, 0.5), r=0.2), State(2., p=1.)), (Box(x=(0.4, 0.9)), State(3., u=0.5, p=2.))]
    base = digest(Problem("p", State(1., p=1.), two))
    assert base == digest(Problem("another name", State(1., p=1.), two))            # the name is the header's "test", not the digest's
    assert base != digest(Problem("p", State(1., p=1.), two[::-1]))                 # the order of the regions decides overlaps
    one_bit = [(two[0][0], State(np.nextafter(2., 3.), p=1.)), two[1]]
    assert base != digest(Problem("p", State(1., p=1.), one_bit))                   # one bit of one state
    assert base != digest(Problem("p", State(1., v=5e-324, p=1.), two))
    assert base != digest(Problem("p", State(1., p=1.), two, gamma=5 / 3))
    assert base != digest(Problem("p", State(1., p=1.), two, samples=2))
    assert base != digest(Problem("p", State(1., p=1.), two, boundaries="FreeFlow"))
    assert base != digest(Problem("p", State(1., p=1.), two), data_type="float32")  # other values reach the device
    assert digest(Problem("p", State(1., p=1.), [(Disc((0.5, 0.5), r=0.25), State(2., p=1.))])) \
        == digest(Problem("p", State(1., p=1.), [(Disc((0.5, 0.5), r2=0.0625), State(2., p=1.))]))


def test_the_digest_of_arrays_is_that_of_their_values():
    rho = np.ones((16, 16))
    z = np.zeros((16, 16))
    a = digest(Problem.from_arrays(rho, z, z, p=rho))
    assert a == digest(Problem.from_arrays(rho.copy(), z, z, p=rho))
    changed = rho.copy()
    changed[3, 5] = np.nextafter(1., 2.)
    assert a != digest(Problem.from_arrays(changed, z, z, p=rho))
    assert a != digest(Problem.from_arrays(rho, z, z, E=rho))


def test_arrays_are_checked():
    ok, z = np.ones((12, 10)), np.zeros((12, 10))
    ArmonParameters(test=Problem.from_arrays(ok, z, z, p=ok), N=(10, 12))
    with pytest.raises(SolverException, match="shape"):
        ArmonParameters(test=Problem.from_arrays(ok, z, z, p=ok), N=(12, 10))
    with pytest.raises(SolverException, match="shape"):
        Problem.from_arrays(ok, z[:, :5], z, p=ok)
    with pytest.raises(SolverException, match="exactly one"):
        Problem.from_arrays(ok, z, z)
    for bad in (float("nan"), 0., -1.):
        rho = ok.copy()
        rho[7, 2] = bad
        with pytest.raises(SolverException, match="rho"):
            Problem.from_arrays(rho, z, z, p=ok)
    u = z.copy()
    u[0, 0] = float("inf")
    with pytest.raises(SolverException, match="NaN or an infinity"):
        Problem.from_arrays(ok, u, z, E=ok)


def test_which_problems_have_an_exact_solution():
    from armon_amd import analytic
    sod = (State(1., E=2.5), State(0.125, E=2.0))
    params = ArmonParameters(test=Problem.riemann(*sod), N=(100, 4))
    assert params.test.riemann_setup() == ("x", 0.5, (1.0, 0.0, (7 / 5 - 1) * 1.0 * 2.5), (0.125, 0.0, (7 / 5 - 1) * 0.125 * 2.0))
    built_in = analytic.reference_for(ArmonParameters(test="Sod", N=(100, 4)), 0.1)
    mine = analytic.reference_for(params, 0.1)
    assert (mine.coord, mine.centre, mine.riemann.speeds, mine.riemann.p_star) == (built_in.coord, built_in.centre, built_in.riemann.speeds, built_in.riemann.p_star)
    assert analytic.reference_for(ArmonParameters(test=Problem.riemann(*sod, axis="y", at=0.25), N=(4, 100)), 0.1).centre == (0.0, 0.25)
    flipped = ArmonParameters(test=Problem("flipped", sod[0], [(HalfPlane((-2, 0), -1.), sod[1])]), N=(100, 4)).test.riemann_setup()
    assert flipped[1] == 0.5 and flipped[2][0] == 1.0 and flipped[3][0] == 0.125        # x >= 0.5 holds the region: it is the right state
    with pytest.raises(SolverException, match="reached a wall"):
        analytic.reference_for(params, 5.0)
    for other in (Problem.riemann(*sod, gamma=5 / 3), implosion(), Problem.riemann(State(1., v=0.1, E=2.5), sod[1]),
                  Problem("two", sod[1], [(HalfPlane((1, 0), 0.5), sod[0]), (HalfPlane((1, 0), 0.2), sod[0])]),
                  Problem("disc", sod[1], [(Disc((0.5, 0.5), r=0.3), sod[0])])):
        p = ArmonParameters(test=other, N=(16, 16))
        assert p.test.riemann_setup() is None and not analytic.has_closed_form(p.test)
        with pytest.raises(SolverException, match="no closed-form"):
            analytic.reference_for(p, 0.1)
        with pytest.raises(SolverException, match="no closed form"):
            ArmonParameters(test=other, N=(16, 16), error_norms_at_end=True)
    # a problem is judged by what it holds, never by its name
    named = ArmonParameters(test=Problem("Sod", sod[1], [(Disc((0.5, 0.5), r=0.3), sod[0])]), N=(16, 16))
    assert not analytic.has_closed_form(named.test)


def test_the_header_of_a_problem_and_of_a_built_in_case():
    from armon_amd import checkpoint
    plain = checkpoint.bit_options(ArmonParameters(test="Sod", N=(16, 16)))
    assert plain["test"] == "Sod" and "gamma" not in plain and "problem_digest" not in plain
    p = ArmonParameters(test=implosion(gamma=5 / 3), N=(16, 16))
    mine = checkpoint.bit_options(p)
    assert mine["test"] == "Problem:implosion" and mine["gamma"] == (5 / 3).hex() and mine["problem_digest"] == p.test.digest
    header = dict(mine, cycle=3, time=(0.01).hex())
    checkpoint.check_compatible(p, header, "file")
    other = ArmonParameters(test=Problem("implosion", State(1., p=1.), [(HalfPlane((1, 1), 0.15), State(np.nextafter(0.125, 1.), p=0.14))],
                                         domain_size=(0.3, 0.3), samples=4, gamma=5 / 3), N=(16, 16))
    with pytest.raises(SolverException, match="problem_digest"):
        checkpoint.check_compatible(other, header, "file")
    with pytest.raises(SolverException, match="test = 'Problem:implosion'"):
        checkpoint.check_compatible(ArmonParameters(test="Sod", N=(16, 16), domain_size=(0.3, 0.3), cfl=0.5), header, "file")


def test_the_ctypes_table_of_a_problem():
    from armon_amd import _lib
    from armon_amd.problem import region_table
    t = ArmonParameters(test=Problem("p", State(1., p=1.), [(Ellipse((0.5, 0.25), (0.2, 0.1)), State(3., u=0.5, E=2.))]), N=(16, 16),
                        data_type="float32").test
    bg, n, regions = region_table(t, np.float32)
    assert n == 1 and isinstance(regions[0], _lib.RegionF32) and list(bg) == [float(v) for v in t.background]
    f = np.float32
    assert regions[0].kind == R.ELLIPSE and list(regions[0].a) == [0.5, 0.25, float(f(1) / (f(0.2) * f(0.2))), float(f(1) / (f(0.1) * f(0.1)))]
    assert (regions[0].rho, regions[0].u, regions[0].v, regions[0].E) == (3., 0.5, 0., 2.)
    import ctypes
    assert ctypes.sizeof(_lib.Region) == 72 and ctypes.sizeof(_lib.RegionF32) == 40


# ---- the restatement on hand-worked cells ------------------------------------------------------------------------------------
A, B, BG = (2., 0.5, 0., 3.), (4., 0., 1., 1.5), (1., 0., 0., 1.)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_centre_exactly_on_a_boundary_is_inside(dtype):
    """N = 16 on the unit domain: the centre of cell 8 is 0.53125 exactly, in both precisions."""
    gx, gy = np.arange(16), np.arange(1)
    for kind, a in ((R.HALF_PLANE, (1., 0., 0.53125, 0.)), (R.BOX, (-np.inf, 0.53125, -np.inf, np.inf)), (R.BOX, (0., 0.53125, 0.03125, 0.03125)),
                    (R.DISC, (0.03125, 0.03125, 0.25, 0.)), (R.ELLIPSE, (0.03125, 0.03125, 4., 1.))):
        rho, u, v, E, mixed = R.restate(gx, gy, (0., 0.), (1 / 16, 1 / 16), 1, BG, [(kind, a, A)], dtype)
        assert rho.dtype == np.dtype(dtype) and not mixed.any()
        assert rho[0].tolist() == [2.] * 9 + [1.] * 7, (kind, rho[0])            # cells 0 .. 8 inside, 8 on the boundary itself
        assert u[0].tolist() == [0.5] * 9 + [0.] * 7 and E[0].tolist() == [3.] * 9 + [1.] * 7
    # exclusive on the other side of the same boundary: x >= 0.53125 written as -x <= -0.53125
    rho = R.restate(gx, gy, (0., 0.), (1 / 16, 1 / 16), 1, BG, [(R.HALF_PLANE, (-1., 0., -0.53125, 0.), A)], dtype)[0]
    assert rho[0].tolist() == [1.] * 8 + [2.] * 8


def test_the_last_region_wins():
    gx, gy = np.arange(4), np.arange(4)
    everywhere = (R.BOX, (-np.inf, np.inf, -np.inf, np.inf))
    left = (R.HALF_PLANE, (1., 0., 0.5, 0.))
    rho = R.restate(gx, gy, (0., 0.), (0.25, 0.25), 1, BG, [everywhere + (A,), left + (B,)], "float64")[0]
    assert rho.tolist() == [[4., 4., 2., 2.]] * 4
    rho = R.restate(gx, gy, (0., 0.), (0.25, 0.25), 1, BG, [left + (B,), everywhere + (A,)], "float64")[0]
    assert rho.tolist() == [[2.] * 4] * 4
    rho = R.restate(gx, gy, (0., 0.), (0.25, 0.25), 1, BG, [], "float64")[0]
    assert rho.tolist() == [[1.] * 4] * 4
    assert R.owner([everywhere + (A,), left + (B,)], np.array([0.1, 0.9]), np.array([0.5, 0.5]), np.float64).tolist() == [1, 0]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_mixed_cell_gives_the_written_quotients(dtype):
    """One cell [0, 1]², samples = 2: the points (0.25 | 0.75)². B holds x >= 0.5 and y >= 0.5 — one sample, the last of the walk."""
    T = np.dtype(dtype).type
    regions = [(R.BOX, (-np.inf, np.inf, -np.inf, np.inf), A), (R.BOX, (0.5, np.inf, 0.5, np.inf), B)]
    rho, u, v, E, mixed = R.restate([0], [0], (0., 0.), (1., 1.), 2, BG, regions, dtype)
    assert mixed.all()
    a, b = [T(x) for x in A], [T(x) for x in B]
    m = ((T(0) + a[0]) + a[0]) + a[0] + b[0]
    mu = ((T(0) + a[0] * a[1]) + a[0] * a[1]) + a[0] * a[1] + b[0] * b[1]
    mv = ((T(0) + a[0] * a[2]) + a[0] * a[2]) + a[0] * a[2] + b[0] * b[2]
    mE = ((T(0) + a[0] * a[3]) + a[0] * a[3]) + a[0] * a[3] + b[0] * b[3]
    assert (rho[0, 0], u[0, 0], v[0, 0], E[0, 0]) == (m / T(4), mu / m, mv / m, mE / m)
    assert (rho[0, 0], u[0, 0], v[0, 0], E[0, 0]) == (T(2.5), T(3) / T(10), T(4) / T(10), T(24) / T(10))
    # mass, momentum and total energy of the cell are those of its four quarters
    assert float(rho[0, 0]) * 4 == 3 * A[0] + B[0]
    # the same cell with one sample: the centre (0.5, 0.5) lies on B's boundary, inside
    one = R.restate([0], [0], (0., 0.), (1., 1.), 1, BG, regions, dtype)
    assert not one[4].any() and [float(f[0, 0]) for f in one[:4]] == list(B)
    # samples of the same region in different places do not make a cell mixed: its state is stored verbatim
    same = R.restate([0], [0], (0., 0.), (1., 1.), 4, BG, regions[:1], dtype)
    assert not same[4].any() and [float(f[0, 0]) for f in same[:4]] == list(A)


def test_the_sample_points():
    """samples = 1 is init_test's x + dX / 2; the points of N = 16 on the unit domain are exact."""
    for T in (np.float64, np.float32):
        gx = np.arange(-4, 20)
        x = gx.astype(T) * T(1 / 16) + T(0)
        assert ((x + T(1 / 16) * T(0.5)) == (x + T(1 / 16) / T(2))).all()
        assert ((x + T(1 / 16) * T(0.5)).astype(np.float64) == (gx + 0.5) / 16).all()
    rho, _, _, _, mixed = R.restate(np.arange(16), [0], (0., 0.), (1 / 16, 1 / 16), 4, BG, [(R.HALF_PLANE, (1., 0., 0.53125, 0.), A)], "float64")
    # cell 8 = [0.5, 0.5625]: its sample columns 0.5078125, 0.5234375 lie inside, 0.5390625, 0.5546875 outside
    assert mixed[0].tolist() == [False] * 8 + [True] + [False] * 7 and rho[0, 8] == 1.5
    gx, gy = R.block((5, 3), 2, (10, 20))
    assert gx.tolist() == list(range(8, 17)) and gy.tolist() == list(range(18, 25))
