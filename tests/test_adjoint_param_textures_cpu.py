"""The reference side of tests/test_gpu_adjoint_param_textures.py (test 1), on the oracle alone: the conditions under which the GPU test
cannot pass vacuously, and the layout of the 2 x 9 maps, by host arithmetic."""
import numpy as np
import pytest

import param_texel_scenes as pts
from test_gpu_textured_params import _box_texcoords

F32 = np.float32


@pytest.mark.parametrize("case", pts.SPLIT_CASES)
def test_oracle_gradients_are_not_small_and_cells_differ(oracle, case):
    """every component of the constant-parameter adjoint of both cells is well above the absolute term of the tolerance (1e-5), and the
    two cells have different gradients: a kernel that mixed the cells up, or scattered nothing, fails the GPU test"""
    film, wants = pts.oracle_wants(case)
    assert np.isfinite(film).all() and film[..., 4].min() > 0
    for key, want in wants.items():
        assert np.isfinite(want) and abs(want) > 1e-3, (case, key, want)
    for (pname, cell, comp), want in wants.items():
        if cell == 0:
            other = wants[(pname, 1, comp)]
            assert abs(want - other) > 2e-3 * max(abs(want), abs(other)) + 1e-5, (case, pname, comp, want, other)


def test_every_lookup_interpolates_equal_texels():
    """u * 8 of the box's texcoords lies in [1, 3] (faces 0-2) or [5, 7] (faces 3-5) and v * 1 in [0, 1): the bilinear footprint of any
    point of a face (a convex combination of its corners) reads columns 1..4 or 5..8 and both rows -- texels that are equal within a
    cell of the 2 x 9 map -- and never column 0.  The arithmetic is that of eval_reflectance (identity to_uv), in float32."""
    uv = _box_texcoords().reshape(6, 4, 2)
    w, h = 9, 2
    m = pts.split_map(0.0, 1.0)
    assert m.shape == (h, w, 3) and np.array_equal(m[0], m[1])
    for face in range(6):
        cell = 0 if face < 3 else 1
        cols = pts.CELL_COLUMNS[cell]
        for u, v in uv[face]:
            ux = F32(F32(u) - np.floor(F32(u))) * F32(w - 1)
            uy = F32(F32(v) - np.floor(F32(v))) * F32(h - 1)
            assert (1.0 <= ux <= 3.0) if cell == 0 else (5.0 <= ux <= 7.0), (face, ux)
            px, py = min(int(ux), w - 2), min(int(uy), h - 2)
            assert py == 0 and px >= 1                                    # column 0 is never part of a footprint
            assert cols.start <= px and px + 1 < cols.stop, (face, px)     # both columns of the footprint lie inside the cell
            assert np.all(m[:, px] == m[:, px + 1]) and np.all(m[:, px] == F32(cell))
    # the extreme columns a lookup can reach: u * 8 = 3 reads (3, 4), u * 8 = 7 reads (7, 8)
    assert pts.CELL_COLUMNS[0].stop == 5 and pts.CELL_COLUMNS[1] == slice(5, 9)
