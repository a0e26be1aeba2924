"""Boundary types of the sides of the domain: the reference's two (ref src/tests.jl:124, ``test_cases``) and ``"Periodic"``,
which has no reference counterpart: problems and the ``periodic`` option only, no built-in case."""
from ._lib import solver_error
from .test_cases import Dirichlet, FreeFlow

Periodic = "Periodic"
BOUNDARY_TYPES = (Dirichlet, FreeFlow, Periodic)


def periodic_axes(boundaries):
    """``(x, y)``: the axes whose two sides (left, right / bottom, top) are ``"Periodic"``. One periodic side facing a side
    of another type is a configuration error that names the axis."""
    axes = []
    for name, (lo, hi) in (("x", boundaries[0:2]), ("y", boundaries[2:4])):
        if (lo == Periodic) != (hi == Periodic):
            solver_error("config", f"boundaries: the two sides of the {name} axis must be periodic together, got "
                                   f"{lo!r} and {hi!r}")
        axes.append(lo == Periodic)
    return tuple(axes)
