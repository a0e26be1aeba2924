"""The history sample on blocks that outgrow the y extent of a launch grid, or whose rows hold thousands of spans, against
the rule in Python, word for word. The shapes are those of tests/test_gpu_long_blocks.py:

 ==== ================ ==========================================================================================
 T1   (10, 65541, 5)   more rows than 65535; odd ghost width: the element path
 T2   (10, 262147, 4)  262147 (row, span) items for at most 3 x CUs workgroups: every wave strides many times
 W1   (300007, 6, 5)   odd pitch; 2344 spans per row (1172 in fp32), a ragged last span
 W2   (300008, 6, 4)   the same with an even pitch: the 16-byte path
 ==== ================ ==========================================================================================

The sample walks a 1-D grid with 64-bit item numbers, so no row or span may be dropped or counted twice: one cell planted in
row 0, 65534, 65535, 65536 and the last row (column 0, 119, 120, 299999 and the last column of a wide block) carries an
extremum of its own, and the record must name exactly that cell.
"""
import numpy as np
import pytest

from test_gpu_history import STATE, fields_of, oracle_record, random_block, same_words

pytestmark = pytest.mark.gpu

SHAPES = dict(T1=(10, 65541, 5), T2=(10, 262147, 4), W1=(300007, 6, 5), W2=(300008, 6, 4))
ROWS = (0, 65534, 65535, 65536, -1)
COLUMNS = (0, 119, 120, 299999, -1)


def positions(name):
    nx, ny, _g = SHAPES[name]
    if ny > nx:
        return [(r % nx, r % ny) for r in ROWS]
    return [(c % nx, c % ny) for c in COLUMNS]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_history_sample_of_a_long_block(name, dtype):
    nx, ny, g = SHAPES[name]
    grid, _ = random_block((nx, ny), g, dtype, "Sod", seed=21)
    host = grid.device_to_host(STATE)
    real = {k: grid.real_view(host[k]) for k in STATE}
    pos = positions(name)
    # five extrema, each decided by one planted cell (draw_state: rho in [0.1, 2], |u|, |v| <= 1, E in [2, 4])
    real["rho"][pos[0][1], pos[0][0]] = 3.0                 # rho_max
    real["rho"][pos[1][1], pos[1][0]] = 0.05                # rho_min
    real["u"][pos[2][1], pos[2][0]] = -2.0                  # speed_max (with E = 8: e stays between the two below)
    real["E"][pos[2][1], pos[2][0]] = 8.0
    real["E"][pos[3][1], pos[3][0]] = 9.0                   # e_max
    real["E"][pos[4][1], pos[4][0]] = 1.75                  # e_min: E - q2 / 2 >= 2 - 1 elsewhere ...
    real["u"][pos[4][1], pos[4][0]] = real["v"][pos[4][1], pos[4][0]] = 1.0     # ... and 0.75 here
    grid.host_to_device(host)
    f = fields_of(grid)
    rec, _ = grid.history_sample()
    assert rec.n == nx * ny and rec.n_bad == 0
    same_words(rec.raw, oracle_record(f, rec.scale_exp), name)
    assert [rec.at[k] for k in ("rho_max", "rho_min", "speed_max", "e_max", "e_min")] == pos
    assert (rec.rho_max, rec.speed_max, rec.e_min) == (3.0, float(np.sqrt(np.float64(4.0) + np.float64(f["v"][pos[2][1], pos[2][0]]) ** 2)), 0.75)
