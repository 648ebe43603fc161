"""Hexagonal cell geometry on the host: what apps/comp_BD/simulate_comp.py uses of the reference's cell/cell.py and
cell/shapes.py -- a Cluster of 1 .. 19 hexagonal ('simple') cells, users placed at random or on a ray towards the border, the
user-to-cell distances, and the wrapped positions of the 19-cell cluster.  The device side (csrc/pipeline_hex.hip:
Engine.hex_gains, Engine.run_hex_drops) takes its tables from here (`hex_tables`).

Positions are complex numbers x + 1j y.  A cell is a hexagon with two horizontal edges: vertices at radius r on 0, 60, ... 300
degrees, height h = sqrt(3) r / 2.  Cell ids count from 1, as in the reference.

Not covered, refused with the reference's error types: Cell3Sec and CellSquare clusters (RuntimeError
"Invalid cell type"), a cluster rotation, Grid with more than its first cluster, wrap around for anything but 19 cells
(RuntimeError); no plotting and no point processes.

    >>> c = Cluster(cell_radius=1.0, num_cells=3)
    >>> [complex(round(p.real, 3), round(p.imag, 3)) for p in c.cell_positions]
    [(-0.5-0.866j), (1+0j), (-0.5+0.866j)]
    >>> round(c.external_radius, 12)
    2.0
"""
import cmath
import itertools
import math
from collections.abc import Iterable

import numpy as np

MAX_CELLS = 19
MAX_ATTEMPTS = 128          # attempts per user of the device's placement ledger

# N = i^2 + i j + j^2: the (i, j) of the cluster sizes that tile the plane; any other size has cluster radius 0
_II_JJ = {1: (1, 0), 3: (1, 1), 4: (2, 0), 7: (2, 1), 13: (3, 1), 19: (3, 2)}

# Wrap around of the 19-cell cluster: cell id -> the (a, b) pairs whose wrapped copy of the cell sits at
# position[a] + position[b] (ids from 1; the position cell b has in a 7- or 19-cell cluster centred on cell a).  The 42 copies
# of the reference's three index tables, grouped per wrapped cell in the tables' order.
_WRAP_19 = {
    2: ((15, 13), (17, 16)), 3: ((16, 16), (19, 18)), 4: ((18, 18), (9, 8)), 5: ((8, 8), (11, 10)),
    6: ((13, 12), (10, 10)), 7: ((13, 11), (15, 14)),
    8: ((15, 4), (12, 11), (17, 17)), 9: ((14, 4), (17, 6)), 10: ((17, 5), (14, 13), (19, 19)), 11: ((19, 7), (16, 5)),
    12: ((18, 7), (15, 16), (9, 9)), 13: ((17, 7), (9, 2)), 14: ((8, 2), (17, 18), (11, 11)), 15: ((8, 7), (11, 3)),
    16: ((10, 3), (13, 13), (19, 8)), 17: ((9, 3), (13, 4)), 18: ((13, 3), (15, 15), (9, 10)), 19: ((12, 3), (15, 5)),
}


def cell_height(radius):
    return radius * math.sqrt(3.0) / 2.0


def normalized_cell_positions(num_cells):
    """Centres of the cells of a cluster of unit radius with cell 1 at the origin: the first ring (cells 2 .. 7) at twice the
    height on 30, 90, ... 330 degrees, the second ring (cells 8 .. 19) alternating 3 radii and 4 heights from 0 degrees in
    steps of 30."""
    pos = np.zeros(num_cells, dtype=complex)
    h = cell_height(1.0)
    ring1 = np.linspace(np.pi / 6.0, 11.0 * np.pi / 6.0, 6)
    for i in range(1, min(num_cells, 7)):
        pos[i] = cmath.rect(2 * h, ring1[i - 1])
    ring2 = np.linspace(0, 11 * np.pi / 6.0, 12)
    for i, a, d in zip(range(7, num_cells), ring2, itertools.cycle([3.0, 4 * h])):
        pos[i] = cmath.rect(d, a)
    return pos


def calc_cell_positions(cell_radius, num_cells):
    """Centres of the cells of a cluster whose CENTROID is the origin (for three cells the common vertex)."""
    # (summed down the rows of a two-column array, position and rotation, as the reference does: NumPy adds the rows of such an
    #  array one after the other but a vector pairwise, and the centres must agree to the last bit for placements to)
    table = np.zeros([num_cells, 2], dtype=complex)
    table[:, 0] = normalized_cell_positions(num_cells)
    table = table * cell_radius
    return table[:, 0] - (np.sum(table, axis=0) / num_cells)[0]


def hexagon_vertices(radius):
    """The six vertices about the origin, from the lower left one counter-clockwise (each the previous plus one edge)."""
    v = np.zeros(6, dtype=complex)
    v[0] = complex(-radius / 2.0, -cell_height(radius))
    angles = np.linspace(0, 240, 5) * np.pi / 180.0
    for k in range(5):
        v[k + 1] = v[k] + radius * np.exp(angles[k] * 1j)
    return v


def inside_hexagon(offset, radius):
    """Is the offset from the centre strictly inside the hexagon: |y| < h and sqrt(3) |x| + |y| < 2 h."""
    h = math.sqrt(3.0) * radius / 2.0
    ax, ay = abs(offset.real), abs(offset.imag)
    return bool(ay < h and math.sqrt(3.0) * ax + ay < 2.0 * h)


def _validate_ratio(ratio):
    if ratio == 1.0:
        return 1.0 - 1e-15          # on the border itself a point would test as outside
    if ratio < 0 or ratio > 1:
        raise ValueError("ratio must be between 0 and 1")
    return ratio


class Node:
    """A user: a position and the id of its cell."""

    def __init__(self, pos, cell_id=None, parent_pos=None):
        self.pos = complex(pos)
        self.cell_id = cell_id
        self.parent_pos = parent_pos

    def calc_dist(self, other):
        return abs(self.pos - other.pos)

    @property
    def relative_pos(self):
        return None if self.parent_pos is None else self.pos - self.parent_pos


class Cell(Node):
    """One hexagonal cell with its users."""

    def __init__(self, pos, radius, cell_id=None, rotation=0):
        super().__init__(pos, cell_id)
        if complex(rotation) != 0:
            raise NotImplementedError("rotated cells are not covered")
        self.radius = float(radius)
        self.id = cell_id
        self.rotation = 0.0
        self._users = []

    height = property(lambda self: cell_height(self.radius))
    users = property(lambda self: self._users)
    num_users = property(lambda self: len(self._users))

    @property
    def vertices(self):
        return self.pos + hexagon_vertices(self.radius) * np.exp(1j * 0.0)

    def is_point_inside_shape(self, point):
        return inside_hexagon(complex(point) - self.pos, self.radius)

    def delete_all_users(self):
        self._users = []

    def add_user(self, new_user, relative_pos_bool=True):
        if not isinstance(new_user, Node):
            raise TypeError("User must be Node object.")
        if relative_pos_bool:
            new_user.pos = new_user.pos * self.radius + self.pos
        if not self.is_point_inside_shape(new_user.pos):
            raise ValueError("User position is outside the cell -> User not added")
        new_user.parent_pos, new_user.cell_id = self.pos, self.id
        self._users.append(new_user)

    def get_border_point(self, angle, ratio=None):
        """The point at `ratio` of the way from the centre to where the ray on `angle` (degrees) meets the border."""
        if ratio is None:
            ratio = 1.0
        rad = np.pi * angle / 180.0
        probe = self.pos + self.radius * np.exp(rad * 1j)
        verts = self.vertices
        near = verts[np.argsort(np.abs(verts - probe))[:2]]          # the edge the ray leaves through
        diff = near[0] - near[1]
        if abs(diff.real) <= 1e-15 * self.radius:                    # (an unrotated hexagon has no such edge; rotation is not covered)
            raise NotImplementedError("a vertical edge needs a rotated cell, which is not covered")
        slope = diff.imag / diff.real
        cut = near[1].imag - slope * near[1].real
        direction = np.exp(1j * rad)
        step = (self.pos.real * slope + cut - self.pos.imag) / (direction.imag - slope * direction.real)
        border = self.pos + np.exp(1j * rad) * step
        return (1 - ratio) * self.pos + ratio * border

    def add_border_user(self, angles, ratio=None):
        if not isinstance(angles, Iterable):
            angles = [angles]
        if ratio is None:
            ratios = itertools.repeat(None)
        elif isinstance(ratio, Iterable):
            ratios = [_validate_ratio(r) for r in ratio]
        else:
            ratios = itertools.repeat(_validate_ratio(float(ratio)))
        for a, r in zip(angles, ratios):
            self._users.append(Node(self.get_border_point(a, r), cell_id=self.id, parent_pos=self.pos))

    def _candidate(self, uniform):
        x = 2 * (uniform() - 0.5) * self.radius
        y = 2 * (uniform() - 0.5) * self.radius
        return self.pos + complex(x, y)

    def add_random_user(self, min_dist_ratio=0.0, uniform=None):
        """A user at a uniform point of the cell at least min_dist_ratio radii from its centre: candidates from the square
        about the cell (two uniforms each, x first) until one is inside.  `uniform`: a callable returning the next uniform
        (default numpy.random.random_sample, as the reference)."""
        uniform = np.random.random_sample if uniform is None else uniform
        pos = self._candidate(uniform)
        while not self.is_point_inside_shape(pos) or abs(self.pos - pos) < min_dist_ratio * self.radius:
            pos = self._candidate(uniform)
        self.add_user(Node(pos, cell_id=self.id, parent_pos=self.pos), relative_pos_bool=False)

    def add_random_users(self, num_users, min_dist_ratio=0.0, uniform=None):
        for _ in range(num_users):
            self.add_random_user(min_dist_ratio, uniform)


class Cluster:
    """1 .. 19 hexagonal cells around `pos` (the centroid of their centres)."""

    def __init__(self, cell_radius, num_cells, pos=0 + 0j, cluster_id=None, cell_type="simple", rotation=0.0):
        if cell_type != "simple":
            raise RuntimeError("Invalid cell type: '{0}'".format(cell_type))
        if rotation not in (None, 0, 0.0):
            raise NotImplementedError("cluster rotation is not covered")
        if not 1 <= int(num_cells) <= MAX_CELLS:
            raise ValueError("num_cells must be in [1, %d] (got %r)" % (MAX_CELLS, num_cells))
        self.pos = complex(pos)
        self.cluster_id = cluster_id
        self.rotation = 0.0
        self._cell_radius = float(cell_radius)
        positions = calc_cell_positions(self._cell_radius, int(num_cells)) + self.pos
        self._cells = [Cell(p, self._cell_radius, i + 1) for i, p in enumerate(positions)]
        self._cell_pos = [np.array([c.pos]) for c in self._cells]      # per cell: its centre, then its wrapped copies
        ii, jj = _II_JJ.get(int(num_cells), (0, 0))
        h = self.cell_height
        self.radius = abs(h * ((jj * 0.5) + (1j * jj * math.sqrt(3.0) / 2.0)) + h * ii)
        self.external_radius = float(np.max(np.abs(self._cells[-1].vertices - self.pos)))

    num_cells = property(lambda self: len(self._cells))
    cell_radius = property(lambda self: self._cell_radius)
    cell_height = property(lambda self: cell_height(self._cell_radius))
    num_users = property(lambda self: sum(c.num_users for c in self._cells))
    cell_positions = property(lambda self: np.array([c.pos for c in self._cells]))

    def __iter__(self):
        return iter(self._cells)

    def calc_dist(self, other):
        return abs(self.pos - other.pos)

    def get_cell_by_id(self, cell_id):
        if cell_id > self.num_cells or cell_id < 1:
            raise ValueError("Invalid cell ID: {0}".format(cell_id))
        return self._cells[cell_id - 1]

    def get_all_users(self):
        return [u for c in self._cells for u in c.users]

    def delete_all_users(self, cell_id=None):
        if isinstance(cell_id, Iterable):
            for i in cell_id:
                self.get_cell_by_id(i).delete_all_users()
        elif cell_id is None:
            for c in self._cells:
                c.delete_all_users()
        else:
            self.get_cell_by_id(cell_id).delete_all_users()

    def add_random_users(self, cell_ids=None, num_users=1, min_dist_ratio=0.0, uniform=None):
        """num_users users in each of the cells `cell_ids` (all cells by default); num_users and min_dist_ratio may be
        iterables that go with cell_ids."""
        if cell_ids is None:
            cell_ids = range(1, self.num_cells + 1)
        if not isinstance(cell_ids, Iterable):
            cell_ids = [cell_ids]
        nums = num_users if isinstance(num_users, Iterable) else itertools.repeat(num_users)
        ratios = min_dist_ratio if isinstance(min_dist_ratio, Iterable) else itertools.repeat(min_dist_ratio)
        for cid, n, ratio in zip(cell_ids, nums, ratios):
            self.get_cell_by_id(int(cid)).add_random_users(int(n), float(ratio), uniform)

    def add_border_users(self, cell_ids, angles, ratios=1.0):
        """Users on the rays `angles` (degrees) at `ratios` of the way to the border; with several cell ids, angles and ratios
        may be iterables that go with them (an entry of angles may itself be a list: several users in that cell)."""
        if not isinstance(cell_ids, Iterable):
            self.get_cell_by_id(cell_ids).add_border_user(angles, ratios)
            return
        angles = angles if isinstance(angles, Iterable) else itertools.repeat(angles)
        ratios = ratios if isinstance(ratios, Iterable) else itertools.repeat(ratios)
        for cid, a, r in zip(cell_ids, angles, ratios):
            self.get_cell_by_id(int(cid)).add_border_user(a, r)

    def create_wrap_around_cells(self, include_users_bool=False):
        """The wrapped copies of the cells of a 19-cell cluster: 42 positions, two or three per cell, none for cell 1."""
        if self.num_cells != 19:
            raise RuntimeError("Wrap around not implemented for a cluster with {0} cells.".format(self.num_cells))
        rel = calc_cell_positions(self._cell_radius, 19)
        self._cell_pos = [np.array([c.pos]) for c in self._cells]
        for cid, pairs in _WRAP_19.items():
            copies = [rel[a - 1] + rel[b - 1] + self.pos for a, b in pairs]
            self._cell_pos[cid - 1] = np.append(self._cell_pos[cid - 1], copies)

    @property
    def wrapped_positions(self):
        """Per cell: its centre followed by its wrapped copies (only the centre before create_wrap_around_cells)."""
        return [p.copy() for p in self._cell_pos]

    def calc_dist_all_users_to_each_cell(self):
        """[user, cell]: the distance from every user (cell by cell) to every cell centre."""
        users = np.array([u.pos for u in self.get_all_users()])
        return np.abs(users[:, np.newaxis] - self.cell_positions)

    calc_dist_all_users_to_each_cell_no_wrap_around = calc_dist_all_users_to_each_cell

    def calc_dist_all_users_to_each_cell_wrapped(self):
        """The same with every cell at the nearest of its positions (what the device computes with wrap_around)."""
        users = np.array([u.pos for u in self.get_all_users()])
        return np.stack([np.min(np.abs(users[:, np.newaxis] - p), axis=1) for p in self._cell_pos], axis=1)


class Grid:
    """The reference's Grid as far as simulate_comp.py calls it: one cluster of 2, 3 or 7 cells at the origin."""

    def __init__(self):
        self._clusters = []

    num_clusters = property(lambda self: len(self._clusters))

    def __iter__(self):
        return iter(self._clusters)

    def clear(self):
        self._clusters = []

    def create_clusters(self, num_clusters, num_cells, cell_radius):
        self.clear()
        if num_cells not in (2, 3, 7):
            raise ValueError("The Grid class does not implement the case of clusters with {0} cells".format(num_cells))
        if num_clusters != 1:
            raise NotImplementedError("only the first cluster of a Grid is covered (got num_clusters = %r)" % (num_clusters,))
        self._clusters.append(Cluster(cell_radius, num_cells, 0 + 0j, 1))

    def get_cluster_from_index(self, index):
        return self._clusters[index]


def hex_tables(num_cells, cell_radius, wrap_around=False):
    """What the device's parameter block holds: (positions [n] complex: every cell's centre followed by its wrapped copies,
    start [num_cells + 1]: where each cell's list begins, external_radius, cluster centre)."""
    cluster = Cluster(cell_radius, num_cells)
    if wrap_around:
        cluster.create_wrap_around_cells()
    lists = cluster.wrapped_positions
    start = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32)
    return np.concatenate(lists), start, cluster.external_radius, cluster.pos
