"""Height fields for qrgpu_plant_step_terrain_batch (include/qrgpu.h), numpy only: a few field makers on one grid, stacked into the
[n_fields][ny][nx] float32 array the call takes.

  g = Grid(nx=24, ny=20, x0=-1.2, y0=-0.9, cell=0.11)
  fields = stack([plane(g, 0.2, -0.1) + rough(g, 0.03, seed=1), stairs(g, 0.05, 0.3, 4)])
  desc = qrgpu.terrain_desc(n_fields=len(fields), **g.desc())

Node (i, j) lies at (x0 + i cell, y0 + j cell); a field is indexed [j][i] (x fastest).  The plant's surface is the Catmull-Rom interpolant of
the nodes, so a step or a gap edge is as sharp as the cell allows and overshoots by a few per cent beside it.
"""
import numpy as np


class Grid:
    def __init__(self, nx, ny, x0, y0, cell):
        assert nx >= 2 and ny >= 2 and cell > 0
        self.nx, self.ny, self.x0, self.y0, self.cell = int(nx), int(ny), float(x0), float(y0), float(cell)

    def desc(self):
        """The grid's members of qrgpu_terrain_desc, by name."""
        return dict(nx=self.nx, ny=self.ny, x0=self.x0, y0=self.y0, cell=self.cell)

    def nodes(self):
        """-> x [ny, nx], y [ny, nx] of the nodes, float64 on the float32 origin and cell the device holds."""
        x0, y0, cell = (float(np.float32(v)) for v in (self.x0, self.y0, self.cell))
        return np.meshgrid(x0 + cell * np.arange(self.nx), y0 + cell * np.arange(self.ny))

    @classmethod
    def centred(cls, half=1.0, cell=0.125):
        """A square grid over [-half, half]^2."""
        n = int(round(2 * half / cell)) + 1
        return cls(n, n, -half, -half, cell)


def flat(grid, z=0.0):
    return np.full((grid.ny, grid.nx), z, np.float32)


def plane(grid, slope_x, slope_y):
    """z = slope_x x + slope_y y: the plane through the world origin."""
    x, y = grid.nodes()
    return (slope_x * x + slope_y * y).astype(np.float32)


def stairs(grid, height, width, k):
    """k steps of `height` up along +x, each `width` deep, the first riser at x = 0: level 0 before it, k height beyond the last."""
    x, _ = grid.nodes()
    return (height * np.clip(np.floor(x / width) + 1, 0, k)).astype(np.float32)


def gap(grid, width, depth, at=0.5):
    """A trench of `width` along x and `depth` deep across the whole field, centred at x = at."""
    x, _ = grid.nodes()
    return np.where(np.abs(x - at) < 0.5 * width, -depth, 0.0).astype(np.float32)


def rough(grid, amplitude, seed):
    """Independent node heights, uniform in +-amplitude."""
    return np.random.default_rng(seed).uniform(-amplitude, amplitude, (grid.ny, grid.nx)).astype(np.float32)


def stack(fields):
    """[n_fields][ny][nx] float32, contiguous: what d_height takes."""
    out = np.ascontiguousarray(np.stack([np.asarray(f, np.float32) for f in fields]))
    assert out.ndim == 3
    return out


KINDS = ("flat", "plane", "stairs", "gap", "rough")


def make(kind, arg=None, grid=None):
    """A field by name, with one optional number: plane:SLOPE_X (0.2), stairs:HEIGHT (0.04; 0.3 deep, 4 steps), gap:WIDTH (0.1; 0.1 deep),
    rough:AMPLITUDE (0.01; seed 1).  -> grid, field [ny, nx]"""
    g = Grid.centred() if grid is None else grid
    a = None if arg is None else float(arg)
    if kind == "flat":
        return g, flat(g)
    if kind == "plane":
        return g, plane(g, 0.2 if a is None else a, 0.0)
    if kind == "stairs":
        return g, stairs(g, 0.04 if a is None else a, 0.3, 4)
    if kind == "gap":
        return g, gap(g, 0.1 if a is None else a, 0.1)
    if kind == "rough":
        return g, rough(g, 0.01 if a is None else a, 1)
    raise ValueError("terrain kind %r: one of %s" % (kind, ", ".join(KINDS)))
