"""User-defined problems: an initial state built on the device from a background and a list of regions, or loaded from
arrays, with its own gamma, EOS and boundary types. No reference counterpart in Python or C: the
reference's users add a ``TestCase`` subtype in Julia (ref src/tests.jl).

    implosion = Problem("implosion", State(1., p=1.), [(HalfPlane((1, 1), 0.15), State(0.125, p=0.14))],
                        domain_size=(0.3, 0.3), maxtime=2.5, samples=4)
    armon(ArmonParameters(test=implosion, N=(400, 400)))

A ``Problem`` is a description; ``ArmonParameters`` binds it to the run's data type and cell size (``Problem.bind``), which
is when the values are rounded, a pressure becomes an energy, and the presets whose constants depend on the cell size
(``Problem.like("Sedov")``) are evaluated. The bound problem stands where a ``TestCase`` stands: every consumer reads
``params.test.gamma``, ``.eos``, ``.boundary_condition``. The rule that turns regions into cells is the one of
``armon_hip_init_regions`` (include/armon_hip.h); it reads the GLOBAL position of a cell only, so tiles, ghost widths and
restarts keep their bit-for-bit guarantees.
"""
import ctypes as C
import dataclasses
import hashlib
import json
import math
import numbers

import numpy as np

from ._lib import Region, RegionF32, check, solver_error
from .blocking import Axis, Side
from .boundaries import BOUNDARY_TYPES, Periodic, periodic_axes
from .test_cases import Dirichlet, FreeFlow, TestCase, _known, create_test

HALF_PLANE, BOX, DISC, ELLIPSE = 0, 1, 2, 3        # ARMON_REGION_*
MAX_REGIONS = 32
SAMPLES = (1, 2, 4, 8)
EOS = ("perfect_gas", "bizarrium")
INIT_TAG = 0            # the two-state tag armon_hip_init_test runs with before the state is overwritten (x, y, mask, zeros)


def _number(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.floating, np.integer)):
        solver_error("config", f"{what} must be a number, got {v!r}")
    return float(v)


def _finite(v, what):
    v = _number(v, what)
    if not math.isfinite(v):
        solver_error("config", f"{what} must be finite, got {v!r}")
    return v


def _pair(v, what, finite=True):
    try:
        a, b = v
    except (TypeError, ValueError):
        solver_error("config", f"{what} takes two numbers, got {v!r}")
    conv = _finite if finite else _number
    return conv(a, what), conv(b, what)


def bind_gravity(gravity, T):
    """The body force ``gravity = (gx, gy)`` as the device receives it: two finite numbers rounded to the data
    type ``T`` (a zero of either sign becomes ``0.0``) → a pair of Python floats. Anything else is a configuration error."""
    try:
        gx, gy = gravity
    except (TypeError, ValueError):
        solver_error("config", f"gravity takes two finite numbers (gx, gy), got {gravity!r}")
    out = []
    for g in (gx, gy):
        if isinstance(g, (bool, np.bool_)) or not isinstance(g, (numbers.Real, np.floating, np.integer)) or not math.isfinite(g):
            solver_error("config", f"gravity takes two finite numbers (gx, gy), got {gravity!r}")
        with np.errstate(over="ignore"):
            r = float(T(g))
        if not math.isfinite(r):
            solver_error("config", f"gravity = {gravity!r} is not finite in {np.dtype(T).name}")
        out.append(r if r != 0 else 0.)
    return tuple(out)


def bind_coefficient(value, T, what):
    """A diffusion coefficient as the device receives it: a finite number >= 0 rounded to the data type ``T``
    → a Python float. Anything else is a configuration error that names ``what``."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (numbers.Real, np.floating, np.integer)) \
            or not math.isfinite(value) or value < 0:
        solver_error("config", f"{what} takes a finite number >= 0, got {value!r}")
    with np.errstate(over="ignore"):
        r = float(T(value))
    if not math.isfinite(r):
        solver_error("config", f"{what} = {value!r} is not finite in {np.dtype(T).name}")
    return r if r != 0 else 0.


SCALAR_TRANSPORTS = ("remap", "bounded")     # how the sweeps carry the passive scalars


def check_scalar_transport(word):
    """``word`` if it names a transport rule of the passive scalars; anything else is a configuration error."""
    if not isinstance(word, str) or word not in SCALAR_TRANSPORTS:
        solver_error("config", f"scalar_transport must be one of {SCALAR_TRANSPORTS}, got {word!r}")
    return word


def diffusion_description(nu, chi, scalars):
    """What a checkpoint's header and a problem's digest say about a diffusive run: ``{"nu", "chi", "scalars": {name: D}}`` with
    the floats as hex text — or None when nothing diffuses, and the headers and digests of such runs stay what they were."""
    D = {sc.name: float(sc.diffusivity).hex() for sc in scalars if sc.diffusivity != 0}
    if nu == 0 and chi == 0 and not D:
        return None
    return {"nu": float(nu).hex(), "chi": float(chi).hex(), "scalars": D}


@dataclasses.dataclass(frozen=True)
class BoundTestCase(TestCase):
    """A built-in case bound to a run: the ``TestCase`` of ``create_test`` with the run's body force, rounded to its data type."""
    gravity: tuple = (0., 0.)
    scalars: tuple = ()          # the run's passive scalars (BoundScalar), sampled with samples = 1
    samples: int = 1
    viscosity: float = 0.        # the run's diffusion coefficients, rounded to its data type
    heat_diffusivity: float = 0.


def bind_case(name, dX, T, gravity=(0., 0.), scalars=None, global_grid=None, viscosity=None, heat_diffusivity=None):
    """``create_test(name, dX, T)`` with the body force ``gravity`` of the run (``bind_gravity``) and its passive ``scalars``
    → ``BoundTestCase``; a forced case is not ``conservative``."""
    case = create_test(name, dX, T)
    gravity = bind_gravity(gravity, T)
    kw = {f.name: getattr(case, f.name) for f in dataclasses.fields(case)}
    if gravity != (0., 0.):
        kw["conservative"] = False
    return BoundTestCase(gravity=gravity, scalars=bind_scalars(scalars, T, global_grid),
                         viscosity=bind_coefficient(0. if viscosity is None else viscosity, T, "viscosity"),
                         heat_diffusivity=bind_coefficient(0. if heat_diffusivity is None else heat_diffusivity, T, "heat_diffusivity"),
                         **kw)


class State:
    """``rho, u, v`` and exactly one of the pressure ``p`` and the specific total energy ``E``. With ``p`` the energy is
    ``p / ((gamma - 1) rho) + (u² + v²) / 2``, evaluated in the run's data type when the problem is bound."""

    def __init__(self, rho, u=0., v=0., p=None, E=None):
        if (p is None) == (E is None):
            solver_error("config", f"a State takes exactly one of p and E, got p = {p!r}, E = {E!r}")
        self.rho, self.u, self.v = _finite(rho, "rho"), _finite(u, "u"), _finite(v, "v")
        self.p = None if p is None else _finite(p, "p")
        self.E = None if E is None else _finite(E, "E")
        if not self.rho > 0:
            solver_error("config", f"a State needs rho > 0, got {rho!r}")

    def energy(self, gamma, T=np.float64):
        if self.E is not None:
            return T(self.E)
        rho, u, v, p = T(self.rho), T(self.u), T(self.v), T(self.p)
        return p / ((T(gamma) - T(1)) * rho) + (u * u + v * v) / T(2)

    def values(self, gamma, T=np.float64):
        """(rho, u, v, E) in ``T``."""
        return (T(self.rho), T(self.u), T(self.v), self.energy(gamma, T))

    def __repr__(self):
        tail = f"p={self.p!r}" if self.E is None else f"E={self.E!r}"
        return f"State(rho={self.rho!r}, u={self.u!r}, v={self.v!r}, {tail})"


class HalfPlane:
    """The points with ``normal · (x, y) <= offset``."""
    kind = HALF_PLANE

    def __init__(self, normal, offset):
        self.normal, self.offset = _pair(normal, "the normal of a HalfPlane"), _finite(offset, "the offset of a HalfPlane")
        if self.normal == (0., 0.):
            solver_error("config", "the normal of a HalfPlane must not be zero")

    def row(self, T):
        return (T(self.normal[0]), T(self.normal[1]), T(self.offset), T(0))


class Box:
    """``lo <= x <= hi`` and the same along y; an infinite bound is an open side."""
    kind = BOX

    def __init__(self, x=(-math.inf, math.inf), y=(-math.inf, math.inf)):
        self.x, self.y = _pair(x, "the x bounds of a Box", finite=False), _pair(y, "the y bounds of a Box", finite=False)
        if any(math.isnan(b) for b in self.x + self.y):
            solver_error("config", f"the bounds of a Box must not be NaN, got {x!r}, {y!r}")

    def row(self, T):
        return (T(self.x[0]), T(self.x[1]), T(self.y[0]), T(self.y[1]))


class Disc:
    """The points within ``r`` of ``centre``; ``r2`` gives the squared radius directly (otherwise ``r * r`` in the data type)."""
    kind = DISC

    def __init__(self, centre, r=None, r2=None):
        if (r is None) == (r2 is None):
            solver_error("config", f"a Disc takes exactly one of r and r2, got r = {r!r}, r2 = {r2!r}")
        self.centre = _pair(centre, "the centre of a Disc")
        self.r = None if r is None else _finite(r, "the radius of a Disc")
        self.r2 = None if r2 is None else _finite(r2, "the squared radius of a Disc")
        if (self.r is not None and self.r < 0) or (self.r2 is not None and self.r2 < 0):
            solver_error("config", "the radius of a Disc must be >= 0")

    def row(self, T):
        r2 = T(self.r2) if self.r2 is not None else T(self.r) * T(self.r)
        return (T(self.centre[0]), T(self.centre[1]), r2, T(0))


class Ellipse:
    """The points with ``((x - cx) / rx)² + ((y - cy) / ry)² <= 1``; ``1 / rx²`` and ``1 / ry²`` are rounded on the host."""
    kind = ELLIPSE

    def __init__(self, centre, radii):
        self.centre, self.radii = _pair(centre, "the centre of an Ellipse"), _pair(radii, "the radii of an Ellipse")
        if not (self.radii[0] > 0 and self.radii[1] > 0):
            solver_error("config", f"the radii of an Ellipse must be > 0, got {radii!r}")

    def row(self, T):
        rx, ry = T(self.radii[0]), T(self.radii[1])
        return (T(self.centre[0]), T(self.centre[1]), T(1) / (rx * rx), T(1) / (ry * ry))


SHAPES = (HalfPlane, Box, Disc, Ellipse)

MAX_SCALARS = 4             # ARMON_MAX_SCALARS: a checkpoint holds 8 planes, 4 of them the state
SCALAR_PREFIX = "s:"        # the plane of the scalar <name> in a checkpoint's header, and in BlockGrid.data


class Scalar:
    """A passive scalar φ — a dye, a mixing fraction, a species tag — carried by the flow (the rule in
    include/armon_hip.h). ``background``: φ of every point no region holds; ``regions``: a list of ``(shape, value)`` with the
    shapes of a ``Problem``, of which the LAST one that holds a point gives φ; a cut cell takes the volume mean of its sample
    points (the problem's ``samples``). ``array``: φ as a global ``(NY, NX)`` array of the real cells instead. Values are any
    finite numbers; nothing bounds φ afterwards either (a second-order remap overshoots). ``diffusivity``: the constant D >= 0
    with which φ diffuses; 0 = a purely advected field."""

    def __init__(self, name, background=0., regions=(), array=None, diffusivity=0.):
        if not isinstance(name, str) or name == "":
            solver_error("config", f"the name of a scalar is a non-empty string, got {name!r}")
        if ":" in name:
            solver_error("config", f"the name of a scalar must not contain ':', got {name!r}")
        self.name = name
        self.diffusivity = bind_coefficient(diffusivity, np.float64, f"the diffusivity of the scalar {name!r}")
        self.background = _finite(background, f"the background of the scalar {name!r}")
        self.regions = list(regions)
        if len(self.regions) > MAX_REGIONS:
            solver_error("config", f"scalar {name!r}: {len(self.regions)} regions: at most {MAX_REGIONS} are supported")
        for item in self.regions:
            if not (isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[0], SHAPES)):
                solver_error("config", f"scalar {name!r}: a region is a pair (shape, value), got {item!r}")
            _finite(item[1], f"a value of the scalar {name!r}")
        self.array = None
        if array is not None:
            if self.regions:
                solver_error("config", f"scalar {name!r} takes regions or an array, not both")
            try:
                a = np.ascontiguousarray(array, dtype=np.float64)
            except (TypeError, ValueError):
                solver_error("config", f"scalar {name!r}: the array must hold numbers")
            if a.ndim != 2:
                solver_error("config", f"scalar {name!r} takes a 2-D array (NY, NX), got the shape {a.shape}")
            if not np.isfinite(a).all():
                solver_error("config", f"scalar {name!r}: the array holds a NaN or an infinity")
            self.array = a

    def __repr__(self):
        what = "array" if self.array is not None else f"background={self.background!r}, {len(self.regions)} regions"
        return f"Scalar({self.name!r}, {what})"


def check_scalars(scalars):
    """The scalars of a problem or a run as a list of ``Scalar``: a dict name → array is spelled out; at most ``MAX_SCALARS``,
    no name twice. Anything else is a configuration error."""
    if scalars is None:
        return []
    if isinstance(scalars, dict):
        scalars = [Scalar(name, array=a) for name, a in scalars.items()]
    try:
        scalars = list(scalars)
    except TypeError:
        solver_error("config", f"scalars takes a list of Scalar (or a dict name -> array), got {scalars!r}")
    for sc in scalars:
        if not isinstance(sc, Scalar):
            solver_error("config", f"scalars takes a list of Scalar (or a dict name -> array), got {sc!r}")
    if len(scalars) > MAX_SCALARS:
        solver_error("config", f"{len(scalars)} scalars: at most {MAX_SCALARS} are supported")
    names = [sc.name for sc in scalars]
    for n in names:
        if names.count(n) > 1:
            solver_error("config", f"the scalar {n!r} is given twice")
    return scalars


class BoundScalar:
    """A ``Scalar`` in a run's data type ``T``: ``array`` (NY, NX) in ``T``, or ``background`` and ``table`` = the rows of
    ``armon_hip_init_regions`` with the values in the slot of ρ."""

    def __init__(self, scalar, T, global_grid=None):
        self.name, self.T = scalar.name, T
        self.diffusivity = bind_coefficient(scalar.diffusivity, T, f"the diffusivity of the scalar {scalar.name!r}")
        hx = lambda vals: [float(v).hex() for v in vals]
        with np.errstate(over="ignore"):
            if scalar.array is not None:
                shape = scalar.array.shape
                if global_grid is not None and shape != (int(global_grid[1]), int(global_grid[0])):
                    solver_error("config", f"scalar {self.name!r}: the array has the shape {shape}, the grid N = {tuple(global_grid)} "
                                           f"needs (NY, NX) = {(int(global_grid[1]), int(global_grid[0]))}")
                self.array = scalar.array.astype(T)
                if not np.isfinite(self.array).all():
                    solver_error("config", f"scalar {self.name!r} is not finite in {np.dtype(T).name}")
                self.background, self.table = T(0), []
                h = hashlib.sha256(repr(shape).encode())
                h.update(np.ascontiguousarray(self.array).tobytes())
                self.description = {"name": self.name, "array": h.hexdigest()}
            else:
                self.array = None
                self.background = T(scalar.background)
                self.table = [(shape.kind, shape.row(T), T(value)) for shape, value in scalar.regions]
                if not all(np.isfinite(v) for v in [self.background] + [v for _, _, v in self.table]):
                    solver_error("config", f"scalar {self.name!r} is not finite in {np.dtype(T).name}")
                self.description = {"name": self.name, "background": float(self.background).hex(),
                                    "regions": [[k, hx(a), float(v).hex()] for k, a, v in self.table]}


def bind_scalars(scalars, T, global_grid=None):
    return tuple(BoundScalar(sc, T, global_grid) for sc in check_scalars(scalars))


def _boundaries(b):
    """The four sides (left, right, bottom, top) of ``boundaries``. The constructor's one-word shorthand stays what it was —
    ``"Dirichlet"`` or ``"FreeFlow"`` for all four sides —; periodic sides are named side by side there, so that which axes
    wrap is written out (``all_sides`` spells one word out for the presets, which take ``"Periodic"`` alone too)."""
    if isinstance(b, str) and b == Periodic:
        solver_error("config", f"boundaries: '{Periodic}' is given side by side — four of '{Dirichlet}', '{FreeFlow}', '{Periodic}' "
                               f"(left, right, bottom, top), both sides of an axis together — got {b!r} alone")
    if isinstance(b, str):
        b = (b,) * 4
    try:
        b = tuple(b)
    except TypeError:
        b = ()
    if len(b) != 4 or not all(isinstance(s, str) and s in BOUNDARY_TYPES for s in b):
        solver_error("config", f"boundaries takes '{Dirichlet}', '{FreeFlow}' or four of '{Dirichlet}', '{FreeFlow}', '{Periodic}' "
                               f"(left, right, bottom, top), got {b!r}")
    periodic_axes(b)            # both sides of an axis are periodic together
    return b


def all_sides(b):
    """One word of ``BOUNDARY_TYPES`` spelled out for the four sides; anything else as it is."""
    return (b,) * 4 if isinstance(b, str) and b in BOUNDARY_TYPES else b


class Problem:
    """A problem the solver can run: ``background`` = the ``State`` of every point no region holds, ``regions`` = a list of
    ``(shape, State)`` of which the LAST one that holds a point gives its state. ``samples``: 1, 2, 4 or 8 points per cell
    and axis; a cell whose points do not all fall in the same region takes the conservative mix of their states.
    ``boundaries``: ``"Dirichlet"`` (a reflecting wall) or ``"FreeFlow"`` for all sides, or four of ``"Dirichlet"``,
    ``"FreeFlow"``, ``"Periodic"`` (left, right, bottom, top); the two sides of an axis are periodic together, and a problem
    with periodic sides sets the run's ``periodic``. The presets (``like``, ``riemann``,
    ``four_quadrants``, ``from_arrays``) also take ``"Periodic"`` alone for all four sides. The shapes of ``regions`` do not wrap around a periodic domain: a disc that leaves it on one side does
    not come back in on the other (build such a state with several shapes, or ``from_arrays``).
    ``gravity = (gx, gy)``: a uniform body force, applied as a kick at the end of every cycle; a forced
    problem is not held to energy conservation. ``scalars``: a list of ``Scalar`` — passive fields carried by the flow
    (DESIGN.md §4.14); ``from_arrays`` also takes a dict name → ``(NY, NX)`` array. ``viscosity``, ``heat_diffusivity``: the
    constant kinematic shear viscosity and the diffusivity of the specific internal energy, both >= 0; the
    options of the same names of ``ArmonParameters`` override them. ``scalar_transport``: ``"remap"`` or ``"bounded"``, the rule
    the sweeps carry the scalars with, overridden likewise. ``domain_size``, ``origin``, ``cfl``, ``maxtime``, ``gravity`` are defaults
    the options of ``ArmonParameters`` override."""

    def __init__(self, name, background, regions=(), gamma=7 / 5, eos="perfect_gas", boundaries=Dirichlet, domain_size=(1., 1.),
                 origin=(0., 0.), cfl=0.5, maxtime=0.2, conservative=True, samples=1, gravity=(0., 0.), scalars=(), _deferred=None,
                 _arrays=None, viscosity=0., heat_diffusivity=0., scalar_transport="remap"):
        self.name = str(name)
        self.scalar_transport = check_scalar_transport(scalar_transport)
        self.viscosity = bind_coefficient(viscosity, np.float64, "viscosity")
        self.heat_diffusivity = bind_coefficient(heat_diffusivity, np.float64, "heat_diffusivity")
        self.scalars = check_scalars(scalars)
        self.gravity = bind_gravity(gravity, np.float64)
        self.gamma = _finite(gamma, "gamma")
        if eos not in EOS:
            solver_error("config", f"unknown eos {eos!r}: one of {EOS}")
        if eos == "perfect_gas" and not self.gamma > 1:
            solver_error("config", f"a perfect gas needs gamma > 1, got {gamma!r}")
        self.eos = eos
        self.boundaries = _boundaries(boundaries)
        self.domain_size = _pair(domain_size, "domain_size")
        self.origin = _pair(origin, "origin")
        if not (self.domain_size[0] > 0 and self.domain_size[1] > 0):
            solver_error("config", f"domain_size must be > 0, got {domain_size!r}")
        self.cfl, self.maxtime = _finite(cfl, "cfl"), _finite(maxtime, "maxtime")
        self.conservative = bool(conservative)
        if isinstance(samples, bool) or samples not in SAMPLES:
            solver_error("config", f"samples must be one of {SAMPLES}, got {samples!r}")
        self.samples = int(samples)
        self._deferred, self._arrays, self._cache = _deferred, _arrays, {}
        self.background, self.regions = background, list(regions)
        if _deferred is None and _arrays is None:
            self._check_states(background, self.regions)

    def _check_states(self, background, regions):
        if len(regions) > MAX_REGIONS:
            solver_error("config", f"{len(regions)} regions: at most {MAX_REGIONS} are supported")
        if not isinstance(background, State):
            solver_error("config", f"the background of a Problem is a State, got {background!r}")
        for item in regions:
            if not (isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[0], SHAPES) and isinstance(item[1], State)):
                solver_error("config", f"a region is a pair (shape, State), got {item!r}")
        if self.eos == "bizarrium" and any(s.E is None for s in [background] + [s for _, s in regions]):
            solver_error("config", "with eos = 'bizarrium' every State must be given by E: its pressure is not the perfect gas's")

    # ---- presets ---------------------------------------------------------------------------------------------------------
    @classmethod
    def like(cls, name, boundaries=None):
        """The built-in case ``name`` (Sod, Sod_y, Sod_circ, Bizarrium, Sedov) written as regions: the same constants,
        boundaries, cfl, maxtime, domain and ``conservative`` flag, and so the same bits. ``boundaries``: other sides than
        the case's own (four of them as ``Problem`` takes them, or one word for all sides, e.g. ``"Periodic"``)."""
        case = TestCase(name=name, **_known(name))
        kw = dict(boundaries=case.boundaries if boundaries is None else all_sides(boundaries), domain_size=case.domain_size, origin=case.origin,
                  cfl=case.cfl, maxtime=case.maxtime, conservative=case.conservative, eos=case.eos)
        sod = (State(0.125, E=2.0), State(1., E=2.5))
        if name == "Sod":
            return cls(name, sod[0], [(HalfPlane((1, 0), 0.5), sod[1])], **kw)
        if name == "Sod_y":
            return cls(name, sod[0], [(HalfPlane((0, 1), 0.5), sod[1])], **kw)
        if name == "Sod_circ":
            return cls(name, sod[0], [(Disc((0.5, 0.5), r2=0.09), sod[1])], **kw)
        if name == "Bizarrium":
            return cls(name, State(10000., u=250., E=0.5 * (250. * 250.)),
                       [(HalfPlane((1, 0), 0.5), State(1.42857142857e+4, E=4.48657821135e+6))], **kw)
        if name == "Sedov":
            def sedov(dX, T):
                # ref src/tests.jl:15-19, :112 as test_cases.create_test and csrc/staged_kernels.hip evaluate them
                r = T(float(T(float(np.hypot(T(dX[0]), T(dX[1]))) / math.sqrt(2))))
                e_in = T(float((1 / 1.033) ** 5 / float(T(math.pi) * (r * r))))
                return State(1., E=2.5e-14), [(Disc((0., 0.), r2=float(r * r)), State(1., E=float(e_in)))]
            return cls(name, None, (), _deferred=sedov, **kw)
        solver_error("config", f"the test case {name} cannot be written as regions")

    @classmethod
    def riemann(cls, left, right, axis="x", at=0.5, name="riemann", **options):
        """``left`` where the coordinate along ``axis`` is <= ``at``, ``right`` beyond; walls across the axis and free flow
        along it unless ``boundaries`` says otherwise."""
        if axis not in ("x", "y"):
            solver_error("config", f"the axis of a Riemann problem is 'x' or 'y', got {axis!r}")
        walls = (Dirichlet, Dirichlet, FreeFlow, FreeFlow) if axis == "x" else (FreeFlow, FreeFlow, Dirichlet, Dirichlet)
        options["boundaries"] = all_sides(options.get("boundaries", walls))
        return cls(name, right, [(HalfPlane((1, 0) if axis == "x" else (0, 1), at), left)], **options)

    @classmethod
    def four_quadrants(cls, states, centre=(0.5, 0.5), name="four_quadrants", **options):
        """A two-dimensional Riemann problem: ``states`` = the four ``State`` of the quadrants around ``centre`` in the usual
        numbering — 1 upper right, 2 upper left, 3 lower left, 4 lower right. Free flow on every side by default."""
        try:
            q1, q2, q3, q4 = states
        except (TypeError, ValueError):
            solver_error("config", f"four_quadrants takes four states, got {states!r}")
        cx, cy = _pair(centre, "the centre of the quadrants")
        inf = math.inf
        options["boundaries"] = all_sides(options.get("boundaries", FreeFlow))
        return cls(name, q1, [(Box(x=(-inf, cx), y=(cy, inf)), q2), (Box(x=(-inf, cx), y=(-inf, cy)), q3),
                              (Box(x=(cx, inf), y=(-inf, cy)), q4)], **options)

    @classmethod
    def from_arrays(cls, rho, u, v, p=None, E=None, name="arrays", **options):
        """The initial state as global ``(NY, NX)`` arrays of the real cells, with exactly one of ``p`` and ``E``. They are
        moved into the block or the tiles band by band through the path a restart uses; ghost cells are rebuilt by the
        first cycle as a restart's are."""
        if (p is None) == (E is None):
            solver_error("config", "from_arrays takes exactly one of p and E")
        arrays = {}
        for key, a in (("rho", rho), ("u", u), ("v", v), ("p" if E is None else "E", p if E is None else E)):
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.ndim != 2 or a.shape != np.shape(rho):
                solver_error("config", f"from_arrays takes 2-D arrays (NY, NX) of one shape, got {key} of shape {a.shape}")
            if not np.isfinite(a).all():
                solver_error("config", f"from_arrays: {key} holds a NaN or an infinity")
            arrays[key] = a
        if not (arrays["rho"] > 0).all():
            solver_error("config", "from_arrays: rho <= 0 in at least one cell")
        if options.get("eos") == "bizarrium" and E is None:
            solver_error("config", "with eos = 'bizarrium' the state must be given by E")
        options.pop("samples", None)
        options["scalars"] = check_scalars(options.get("scalars"))
        for sc in options["scalars"]:
            if sc.array is not None and sc.array.shape != np.shape(rho):
                solver_error("config", f"from_arrays: the scalar {sc.name!r} has the shape {sc.array.shape}, the state {np.shape(rho)}")
        if "boundaries" in options:
            options["boundaries"] = all_sides(options["boundaries"])
        return cls(name, None, (), _arrays=arrays, **options)

    # ---- binding ---------------------------------------------------------------------------------------------------------
    def bind(self, dX, T=np.float64, global_grid=None, gravity=None, scalars=None, viscosity=None, heat_diffusivity=None):
        """This problem for a run in the data type ``T`` with cells ``dX`` on ``global_grid = (NX, NY)`` → ``BoundProblem``.
        ``gravity``: the run's own body force instead of the problem's (the ``gravity`` option of ``ArmonParameters``).
        ``scalars``: the run's own passive scalars, after the problem's (the ``scalars`` option)."""
        T = np.dtype(T).type
        gravity = bind_gravity(self.gravity if gravity is None else gravity, T)
        extra = check_scalars(scalars)
        nu = bind_coefficient(self.viscosity if viscosity is None else viscosity, T, "viscosity")
        chi = bind_coefficient(self.heat_diffusivity if heat_diffusivity is None else heat_diffusivity, T, "heat_diffusivity")
        key = (T, float(dX[0]), float(dX[1]), None if global_grid is None else tuple(global_grid), gravity,
               tuple(id(sc) for sc in extra), nu, chi)
        if key not in self._cache:
            self._cache = {key: BoundProblem(self, dX, T, global_grid, gravity, check_scalars(self.scalars + extra), nu, chi)}
            self._cache_scalars = extra        # (keeps the ids of the key alive)
        return self._cache[key]

    def __repr__(self):
        what = "arrays" if self._arrays is not None else "regions by cell size" if self._deferred else f"{len(self.regions)} regions"
        return f"Problem({self.name!r}, {what}, gamma={self.gamma!r}, eos={self.eos!r}, samples={self.samples})"


class BoundProblem:
    """A ``Problem`` in a run's data type: what ``ArmonParameters.test`` holds, with the interface of a ``TestCase``."""
    is_problem = True
    tag = INIT_TAG
    r = 0.

    def __init__(self, problem, dX, T, global_grid, gravity=(0., 0.), scalars=(), viscosity=0., heat_diffusivity=0.):
        P = self.problem = problem
        self.scalars = bind_scalars(scalars, T, global_grid)
        self.viscosity = bind_coefficient(viscosity, T, "viscosity")          # the values the device receives
        self.heat_diffusivity = bind_coefficient(heat_diffusivity, T, "heat_diffusivity")
        self.gravity = bind_gravity(gravity, T)            # the two values the device receives
        self.name, self.header_name = P.name, "Problem:" + P.name
        self.gamma, self.eos, self.boundaries, self.samples = P.gamma, P.eos, P.boundaries, P.samples
        self.domain_size, self.origin, self.cfl, self.maxtime = P.domain_size, P.origin, P.cfl, P.maxtime
        self.conservative = P.conservative and self.gravity == (0., 0.)      # a force does work: total energy is not conserved
        self.T = T
        background, regions = P.background, P.regions
        if P._deferred is not None:
            background, regions = P._deferred(dX, T)
            P._check_states(background, regions)
        self.arrays, arrays_digest = None, None
        if P._arrays is not None:
            self.arrays, arrays_digest = self._bind_arrays(P._arrays, global_grid)
            self.background, self.table = tuple(T(v) for v in (1, 0, 0, 1)), []
        else:
            self.background = background.values(P.gamma, T)
            self.table = [(shape.kind, shape.row(T), state.values(P.gamma, T)) for shape, state in regions]
        for what, state in [("the background", self.background)] + [(f"region {k}", s) for k, (_, _, s) in enumerate(self.table)]:
            if not all(np.isfinite(v) for v in state) or not state[0] > 0:
                solver_error("config", f"{what} is not a finite state with rho > 0 in {np.dtype(T).name}: rho, u, v, E = {state}")
        hx = lambda vals: [float(v).hex() for v in vals]
        self.description = {"gamma": float(P.gamma).hex(), "eos": P.eos, "boundaries": list(P.boundaries), "samples": P.samples,
                            "background": hx(self.background), "regions": [[k, hx(a), hx(s)] for k, a, s in self.table],
                            "arrays": arrays_digest}
        if self.gravity != (0., 0.):                # only then: the digests of the problems without a force stay what they were
            self.description["gravity"] = hx(self.gravity)
        if self.scalars:                            # only then, likewise
            self.description["scalars"] = [sc.description for sc in self.scalars]
        diffusion = diffusion_description(self.viscosity, self.heat_diffusivity, self.scalars)
        if diffusion is not None:                   # only then, likewise
            self.description["diffusion"] = diffusion
        self.digest = hashlib.sha256(json.dumps(self.description, sort_keys=True).encode("utf-8")).hexdigest()

    def _bind_arrays(self, src, global_grid):
        T, T_gamma = self.T, self.T(self.gamma)
        shape = src["rho"].shape
        if global_grid is not None and shape != (int(global_grid[1]), int(global_grid[0])):
            solver_error("config", f"from_arrays: the arrays have the shape {shape}, the grid N = {tuple(global_grid)} needs "
                                   f"(NY, NX) = {(int(global_grid[1]), int(global_grid[0]))}")
        out = {f: src[f].astype(T) for f in ("rho", "u", "v")}
        if "E" in src:
            out["E"] = src["E"].astype(T)
        else:
            rho, u, v, p = out["rho"], out["u"], out["v"], src["p"].astype(T)
            out["E"] = p / ((T_gamma - T(1)) * rho) + (u * u + v * v) / T(2)
        for f, a in out.items():
            if not np.isfinite(a).all() or (f == "rho" and not (a > 0).all()):
                solver_error("config", f"from_arrays: {f} is not finite{' and > 0' if f == 'rho' else ''} in {np.dtype(T).name}")
        h = hashlib.sha256(repr(shape).encode())
        for f in ("rho", "u", "v", "E"):
            h.update(np.ascontiguousarray(out[f]).tobytes())
        return out, h.hexdigest()

    def boundary_condition(self, side):
        """(u_factor, v_factor) for ``side``, as ``TestCase.boundary_condition``. A periodic side has no mirror: no kernel is
        given its factors (the neutral pair stands in the descriptors of its sweeps, which read its ghosts instead)."""
        cond = self.boundaries[int(side) - 1]
        if cond in (FreeFlow, Periodic):
            return (1., 1.)
        return (-1., 1.) if side in (Side.Left, Side.Right) else (1., -1.)

    def riemann_setup(self):
        """When this problem is a one-dimensional perfect-gas Riemann problem the exact solver covers — one axis-aligned
        half-plane, no transverse velocity, gamma = 7/5 — → ``(axis, x0, left, right)`` with the states as (rho, un, p); None
        otherwise."""
        if self.arrays is not None or len(self.table) != 1 or self.table[0][0] != HALF_PLANE:
            return None
        if self.eos != "perfect_gas" or self.gamma != 7 / 5:
            return None
        _, a, inner = self.table[0]
        nx, ny, offset = float(a[0]), float(a[1]), float(a[2])
        if (nx != 0) == (ny != 0):
            return None
        axis, n = ("x", nx) if nx != 0 else ("y", ny)

        def primitive(state):
            rho, u, v, E = (float(s) for s in state)
            un, ut = (u, v) if axis == "x" else (v, u)
            return ut, (rho, un, (self.gamma - 1) * rho * (E - (u * u + v * v) / 2))
        (t_in, s_in), (t_out, s_out) = primitive(inner), primitive(self.background)
        if t_in != 0 or t_out != 0:
            return None
        left, right = (s_in, s_out) if n > 0 else (s_out, s_in)
        return axis, offset / n, left, right

    def __repr__(self):
        return f"BoundProblem({self.header_name!r}, {np.dtype(self.T).name}, digest {self.digest[:12]})"


# ---- the device side -------------------------------------------------------------------------------------------------------
def region_table(test, T):
    """The ctypes arguments of ``armon_hip_init_regions``: (background, n, regions)."""
    real, Reg = (C.c_float, RegionF32) if np.dtype(T) == np.float32 else (C.c_double, Region)
    regions = (Reg * max(len(test.table), 1))()
    for reg, (kind, a, state) in zip(regions, test.table):
        reg.kind = kind
        reg.a = (real * 4)(*[float(x) for x in a])
        reg.rho, reg.u, reg.v, reg.E = (float(s) for s in state)
    return (real * 4)(*[float(s) for s in test.background]), len(test.table), regions


def init_state(params, grid):
    """Overwrite rho, u, v, E of ``grid`` — on which ``armon_hip_init_test`` has just run — with the problem's state."""
    test = params.test
    if test.arrays is not None:
        return _load_arrays(params, grid, test.arrays)
    bs = params.block_size
    full = bs.domain_range(*params.steps_ranges[Axis.X].full_domain).to_c()
    real = C.c_float if params.data_type == np.float32 else C.c_double
    gpos = (C.c_int64 * 2)(params.N_origin[0] - 1, params.N_origin[1] - 1)
    origin = (real * 2)(*params.origin)
    dX = (real * 2)(params.cell_size(0), params.cell_size(1))
    background, n, regions = region_table(test, params.data_type)
    p = grid.ptr
    check(params.fn("init_regions")(params.device.ctx, full, bs.size[0], bs.ghosts, C.byref(gpos), C.byref(origin), C.byref(dX),
                                    test.samples, C.byref(background), n, regions, p("rho"), p("u"), p("v"), p("E")))


def init_scalars(params, grid):
    """The initial planes of the run's passive scalars. A region-built one is what
    ``armon_hip_init_regions`` puts into ρ when the regions' densities are the scalar's values —
    ``armon_hip_init_scalar_regions``, the same device code, with the plane in the slot of ρ and three ping-pong partners of the
    state, which hold nothing before the first sweep, as scratch —; an array is moved in band by band like the state of ``from_arrays``."""
    for sc in params.scalars:
        plane = SCALAR_PREFIX + sc.name
        if sc.array is not None:
            _load_arrays(params, grid, {plane: sc.array}, names=(plane,))
            continue
        bs = params.block_size
        full = bs.domain_range(*params.steps_ranges[Axis.X].full_domain).to_c()
        real, Reg = (C.c_float, RegionF32) if params.data_type == np.float32 else (C.c_double, Region)
        gpos = (C.c_int64 * 2)(params.N_origin[0] - 1, params.N_origin[1] - 1)
        origin = (real * 2)(*params.origin)
        dX = (real * 2)(params.cell_size(0), params.cell_size(1))
        regions = (Reg * max(len(sc.table), 1))()
        for reg, (kind, a, value) in zip(regions, sc.table):
            reg.kind = kind
            reg.a = (real * 4)(*[float(x) for x in a])
            reg.rho, reg.u, reg.v, reg.E = float(value), 0., 0., 0.
        background = (real * 4)(float(sc.background), 0., 0., 0.)
        scratch = [C.c_void_p(grid.alt[f].ptr) for f in ("u", "v", "E")]
        check(params.fn("init_scalar_regions")(params.device.ctx, full, bs.size[0], bs.ghosts, C.byref(gpos), C.byref(origin),
                                               C.byref(dX), int(getattr(params.test, "samples", 1)), C.byref(background),
                                               len(sc.table), regions, grid.ptr(plane), *scratch))


def _load_arrays(params, grid, arrays, names=None):
    """The tile's window of the global arrays, band by band, through ``armon_hip_state_unpack`` (what ``load_state`` uses)."""
    from . import checkpoint
    names = checkpoint.STATE_PLANES if names is None else names
    nx = params.N[0]
    ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
    dev = params.device
    _, bands = checkpoint._bands(params, len(names), None)
    digest = dev.zeros(8, np.uint64)
    try:
        for r0, rows in bands:
            dense = np.stack([arrays[f][oy + r0:oy + r0 + rows, ox:ox + nx] for f in names])      # [4][rows][nx]
            stage = dev.from_host(dense)
            try:
                checkpoint._move(params, grid, names, (0, r0, nx, rows), stage, digest, unpack=True)
            finally:
                stage.free()                # waits for the stream
    finally:
        digest.free()
