"""A board of 1 100 small meshes, for the tests that hold every per-mesh kernel to its restatement where the mesh count, not
the mesh size, is large (tests/test_many_meshes_host.py on the CPU, tests/test_many_meshes.py on the device).  Needs no GPU.

The board (every mesh a synthetic.jittered_grid with jitter 0.2):

  1 056 pads   33 x 32 on a 3 mm pitch, pad k on layer k % 3, its grid SHAPES[(7 k + k // 33) % 8] at h = 0.25; four of them
               are replaced by long grids (SPECIAL) whose vertex or face counts sit on and beside a tile of 256
  the plane    41 x 39 at h = 2.5 on layer 3, under all pads: 12 face tiles, 7 vertex tiles
  43 pads      3 x 3 on layer 3, beside the plane

Mesh order: the pads in k order, the plane right after pad 500, and after every pad with k % 25 == 3 the next of the 43.  Every
pair of consecutive meshes lies on different layers, and the layers have different conductances: a face, vertex or tile
attributed to mesh m - 1 or m + 1 gets another conductance, so the bits of what is computed from it change.

The 2 x 2, 2 x 3 and 3 x 2 pads have no interior vertex and so exact right angles: their diagonal cotangents are exact zeros.

One network: a source of 2 A from the plane's corner into an internal node, from there a resistor to the first pad of each of
the 32 rows, the pads of a row chained from upper right corner to lower left corner, the last one through a via from its upper
right corner to the plane point under its centre (from the centre of a 2 x 2 pad, which snaps to the corner the current came
in at, the pad would carry none); the 43 pads
in a chain of resistors from the plane point (99, 50), a second source of 0.5 A from the plane point nearest (99, 96.5) into
the chain's end.  Every mesh carries current in case 0 (asserted on the oracle's solve by the host test)."""
import math

import numpy as np

import helpers as H
import sensitivity_ref as S
import thermal_ref as T
from oracle import padne_oracle as O
from padne_amd import mesh, problem as P, reduction, solver, synthetic

SHAPES = [(2, 2), (2, 3), (3, 2), (3, 3), (4, 3), (3, 5), (5, 5), (6, 4)]
H_PAD, PITCH, PER_ROW, N_ROWS = 0.25, 3.0, 33, 32
N_PADS = PER_ROW * N_ROWS
SPECIAL = {5: (2, 128), 600: (2, 129), 1055: (9, 17), 333: (4, 44)}        # h = 2 / max(nx, ny)
PLANE = (3, 41, 39, 2.5, (-1.0, -1.0), 7)                                   # layer, nx, ny, h, origin, seed
PLANE_AFTER = 500
N_UNDER = 43
LAYERS = (("F.Cu", 2000.0), ("In1.Cu", 1500.0), ("In2.Cu", 1250.0), ("B.Cu", 1000.0))
N_MESH, N_VERT, N_TRI, FACE_TILES, VERTEX_TILES = 1100, 15_851, 18_266, 1112, 1107
FACES_PER_MESH = {2, 4, 8, 12, 16, 30, 32, 254, 256, 258, 3040}
N_CONNECTIONS, N_ELEMENTS = 2233, 1133


def tiles(n) -> int:
    return -(-int(n) // 256)


def fsum(a) -> float:
    return math.fsum(np.asarray(a, dtype=np.float64).reshape(-1).tolist())


def pad_grid(k):
    """(layer, nx, ny, h, origin, seed) of pad k."""
    nx, ny = SHAPES[(7 * k + k // PER_ROW) % 8]
    h = H_PAD
    if k in SPECIAL:
        nx, ny = SPECIAL[k]
        h = 2.0 / max(nx, ny)
    return k % 3, nx, ny, h, (PITCH * (k % PER_ROW), PITCH * (k // PER_ROW)), 1000 + k


def under_grid(k):
    return 3, 3, 3, H_PAD, (110.0 + PITCH * (k % 7), PITCH * (k // 7)), 5000 + k


def grids():
    """The grids in mesh order, with what each is: ("pad", k), ("plane", 0) or ("under", k)."""
    out, under = [], 0
    for k in range(N_PADS):
        out.append((("pad", k), pad_grid(k)))
        if k == PLANE_AFTER:
            out.append((("plane", 0), PLANE))
        if k % 25 == 3:
            out.append((("under", under), under_grid(under)))
            under += 1
    assert under == N_UNDER
    return out


def corner(grid, right_top):
    _layer, nx, ny, h, (x0, y0), _seed = grid
    return (x0 + (nx - 1) * h, y0 + (ny - 1) * h) if right_top else (x0, y0)


class Board:
    """The board, its Problem, its numbering and its restatement's arrays (what tests/test_many_tiles.py's Wide holds)."""

    def __init__(self):
        self.what, self.grids, self.meshes, self.layer_of = [], [], [], []
        for what, grid in grids():
            layer, nx, ny, h, origin, seed = grid
            xy, tri = synthetic.jittered_grid(nx, ny, h=h, seed=seed, jitter=0.2, origin=origin)
            self.meshes.append(mesh.Mesh(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3)))
            self.what.append(what)
            self.grids.append(grid)
            self.layer_of.append(layer)
        self.mesh_of = {what: m for m, what in enumerate(self.what)}
        self.layers = [P.Layer(shape=H.Geoms(1), name=name, conductance=s) for name, s in LAYERS]
        self.prob, self.sources, elements = self._network()
        self.cases = [{}, {self.sources[0]: 3.4, self.sources[1]: -0.3}, {e: 0.0 for e in self.sources}]
        self.board = solver.index_board(self.prob, self.meshes, self.layer_of)
        nodes = self.board.node_indexer
        self.pairs = solver.global_elements(list(self.prob.networks), nodes)
        self.n_internal = nodes.internal_node_count
        sigma = [self.prob.layers[l].conductance for l in self.layer_of]
        self.system = S.System(meshes=[(m.points, m.triangles, s) for m, s in zip(self.meshes, sigma)], n_internal=self.n_internal,
                               rows=[row for _, row in self.pairs], ground=solver.find_best_ground_node_index(self.prob, nodes),
                               layer_of=self.layer_of, prob=self.prob, pairs=self.pairs, nodes=nodes, flat=elements)
        self.flat = [(np.asarray(m.points, dtype=np.float64), np.asarray(m.triangles, dtype=np.int64)) for m in self.meshes]
        self.xy, self.tri, self.face_mesh, self.voff, self.toff = T.flatten(self.flat)
        self.sigma = np.asarray(sigma, dtype=np.float64)
        self.n_vert, self.n_tri, self.n_mesh = len(self.xy), len(self.tri), len(self.meshes)
        self.n_pot = self.n_vert + self.n_internal
        self.ml = np.asarray(self.layer_of, dtype=np.int32)
        self.face_area = T.face_area(self.xy, self.tri)
        self.M = T.lumped(self.xy, self.tri)
        self._direct = None

    def _network(self):
        at = lambda layer, xy: P.Connection(layer=self.layers[layer], point=H.XY(*xy))      # noqa: E731
        plane = self.grids[self.mesh_of["plane", 0]]
        c, elements = [], []

        def resistor(a, b, ohms):
            c.extend((a, b))
            elements.append(P.Resistor(a=a.node_id, b=b.node_id, resistance=ohms))
        hub = P.NodeID()
        feed = at(3, corner(plane, False))
        c.append(feed)
        sources = [P.CurrentSource(f=feed.node_id, t=hub, current=2.0)]
        for j in range(N_ROWS):
            row = [self.grids[self.mesh_of["pad", PER_ROW * j + i]] for i in range(PER_ROW)]
            first = at(row[0][0], corner(row[0], False))
            c.append(first)
            elements.append(P.Resistor(a=hub, b=first.node_id, resistance=0.05 * (1 + j % 5)))
            for i in range(PER_ROW - 1):
                n = PER_ROW * j + i
                resistor(at(row[i][0], corner(row[i], True)), at(row[i + 1][0], corner(row[i + 1], False)), 0.01 + 0.001 * (n % 5))
            (x0, y0), (x1, y1) = corner(row[-1], False), corner(row[-1], True)
            centre = (0.5 * (x0 + x1), 0.5 * (y0 + y1))
            resistor(at(row[-1][0], (x1, y1)), at(3, centre), 0.002)          # (out at the corner: the current crosses the pad)
        under = [self.grids[self.mesh_of["under", k]] for k in range(N_UNDER)]
        resistor(at(3, (99.0, 50.0)), at(3, corner(under[0], False)), 0.02)
        for k in range(N_UNDER - 1):
            resistor(at(3, corner(under[k], True)), at(3, corner(under[k + 1], False)), 0.02)
        a, b = at(3, (99.0, 96.5)), at(3, corner(under[-1], True))
        c.extend((a, b))
        sources.append(P.CurrentSource(f=a.node_id, t=b.node_id, current=0.5))
        elements = sources + elements
        assert len(c) == N_CONNECTIONS and len(elements) == N_ELEMENTS
        return P.Problem(layers=self.layers, networks=[P.Network(connections=c, elements=elements)]), sources, elements

    def faces(self, m):
        return int(self.toff[m]), int(self.toff[m + 1])

    def verts(self, m):
        return int(self.voff[m]), int(self.voff[m + 1])

    def case_rows(self, case):
        """The element rows with one load case's source values (tests/test_load_case_currents.py::case_rows)."""
        return [tuple(case[e] if p == 3 else v for p, v in enumerate(row)) if e in case else row for e, row in self.pairs]

    def direct(self):
        """(M, R, X): the oracle's matrix, the right-hand sides of the three cases and their direct solves, made once."""
        if self._direct is None:
            import scipy.sparse as sp
            import scipy.sparse.linalg as spla
            M, _ = self.system.assemble()
            R = self._case_rhs(M.shape[0])
            lu = spla.splu(sp.csc_matrix(M))
            self._direct = (M, R, np.stack([lu.solve(R[:, j]) for j in range(R.shape[1])], axis=1))
        return self._direct

    def _case_rhs(self, N):
        """The right-hand sides of the three cases as the oracle stamps a current source (no second assembly of M)."""
        R = np.zeros((N, len(self.cases)))
        for j, case in enumerate(self.cases):
            for row in self.case_rows(case):
                if row[0] == "I":
                    R[row[1], j] += row[3]
                    R[row[2], j] += -row[3]
                else:
                    assert row[0] == "R"
        return R

    # ---- per-mesh values that differ between consecutive meshes by exactly representable factors ------------------------------

    def per_mesh(self, base, mod, parts):
        return [float(base) * (1 + (m % mod) / parts) for m in range(self.n_mesh)]

    # ---- the constraints of the strip-numbering tests ---------------------------------------------------------------------------

    def strip_ties(self):
        """Voltage sources inside 2 x 2 pads (vertices 0 (0, 0), 1 (h, 0), 2 (0, h), 3 (h, h)), as (p, n, volts) on global
        vertices, and the pads by what they leave: two owners above each other (equal x, the degenerate box), two owners side by
        side (equal y), three owners, one owner, and none (all four tied to a vertex of the mesh before)."""
        small = [m for m, (what, grid) in enumerate(zip(self.what, self.grids)) if what[0] == "pad" and grid[1:3] == (2, 2)]
        pick = dict(equal_x=small[3], equal_y=small[40], three=small[77], one=small[101], none=small[120], equal_x_late=small[-2])
        local = dict(equal_x=[(1, 0), (3, 2)], equal_y=[(2, 0), (3, 1)], three=[(3, 2)], one=[(1, 0), (2, 1), (3, 2)],
                     none=[(1, 0), (2, 1), (3, 2)], equal_x_late=[(1, 0), (3, 2)])
        ties = []
        for name, m in pick.items():
            v0 = int(self.voff[m])
            ties += [(v0 + p, v0 + n) for p, n in local[name]]
            if name == "none":
                ties.append((v0, int(self.voff[m - 1])))
        return [(p, n, 1e-4 * (1 + i % 3)) for i, (p, n) in enumerate(ties)], pick

    def tied_rows(self):
        """The element rows of the board with the voltage sources of strip_ties behind them: (rows, ground, pick)."""
        ties, pick = self.strip_ties()
        rows = [row for _, row in self.pairs]
        rows += [("V", p, n, volts, self.n_pot + i) for i, (p, n, volts) in enumerate(ties)]
        return rows, self.system.ground, pick

    def tied_layout(self):
        """The KKT layout of tied_rows: every source's multiplier row behind the potentials, then the ground row."""
        rows, ground, pick = self.tied_rows()
        cons = [reduction.Constraint(index=row[4], p=row[1], n=row[2], value=row[3]) for row in rows if row[0] == "V"]
        N = self.n_pot + len(cons) + 1
        cons.append(reduction.Constraint(index=N - 1, p=ground, n=-1, value=0.0))
        return reduction.KKTLayout(size=N, n_potential=self.n_pot, constraints=cons), pick


def lexsort_order(red, xy, voff):
    """The stated rule of the locality ordering, plainly: the owners (the first vertex of every reduced unknown) sorted by
    (mesh, strip, x quantised to 32 bits inside the mesh's owners), equal keys in index order, the unknowns that are no vertex
    behind them in their old order.  A mesh whose owners' box has zero width or zero height: strip 0.  Returns the permutation
    (new position -> old reduced index) of a Reduction that has NOT been reordered."""
    n_vert = int(voff[-1])
    imap = np.asarray(red.index_map)
    owner = np.full(red.n_free, -1, dtype=np.int64)
    for v in range(n_vert - 1, -1, -1):
        if imap[v] >= 0:
            owner[imap[v]] = v
    has = owner >= 0
    mesh_id = np.where(has, np.searchsorted(voff, np.maximum(owner, 0), side="right") - 1, len(voff))
    strip, xq = np.zeros(red.n_free, dtype=np.int64), np.arange(red.n_free, dtype=np.float64)
    for m in np.unique(mesh_id[has]):
        sel = np.flatnonzero(has & (mesh_id == m))
        x, y = xy[owner[sel], 0], xy[owner[sel], 1]
        width, rise = x.max() - x.min(), y.max() - y.min()
        if len(sel) >= 2 and width != 0.0 and rise != 0.0:
            strip[sel] = np.floor((y - y.min()) / (3.4 * np.sqrt(width * rise / len(sel)))).astype(np.int64)
        xq[sel] = np.floor(np.minimum((x - x.min()) / max(width, 1e-300) * (2.0 ** 32 - 1), 2.0 ** 32 - 1))
    return np.lexsort((xq, strip, mesh_id)), owner, mesh_id
