"""CPU: pyphysim_amd.cell (the host geometry of the hexagonal cluster) and tests/hex_oracle.py against the reference's own
results (tests/golden/g9_hex.npz, written by scripts/make_golden_hex.py); the placement ledger; what is refused; the argument
rules of CompSimulator's user positioning."""
import itertools

import numpy as np
import pytest

import hex_oracle as ho
from pyphysim_amd import _lib, cell, pathloss

RTOL = 1e-13


@pytest.fixture(scope="module")
def fx():
    return dict(ho.load_fixture())


def close(got, want, rtol=RTOL):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= rtol * np.maximum(np.abs(want), 1e-300)))


def place_cases(fx):
    c = 0
    while "place%d_cfg" % c in fx:
        K, U, ratio, r, S = fx["place%d_cfg" % c]
        yield c, int(K), int(U), float(ratio), float(r), int(S)
        c += 1


# ---- geometry ----------------------------------------------------------------------------------------------------------
def test_cluster_geometry_against_the_reference(fx):
    for (k, K), (i, r) in itertools.product(enumerate(fx["geo_cells"]), enumerate(fx["geo_radii"])):
        cl = cell.Cluster(float(r), int(K))
        key = "geo%d_%d_" % (k, i)
        scale = np.max(np.abs(fx[key + "vlast"]))
        assert np.max(np.abs(cl.cell_positions - fx[key + "centres"])) <= RTOL * scale, (K, r)
        cells = list(cl)
        # the reference's vertex order: entry by entry, not as a set
        assert np.max(np.abs(cells[0].vertices - fx[key + "vfirst"])) <= RTOL * scale
        assert np.max(np.abs(cells[-1].vertices - fx[key + "vlast"])) <= RTOL * scale
        assert close([cl.radius, cl.external_radius, cl.cell_height], fx[key + "radii"]) or (
            fx[key + "radii"][0] == 0 and cl.radius == 0 and close([cl.external_radius, cl.cell_height], fx[key + "radii"][1:]))
        assert cl.num_cells == K and cl.cell_radius == r and [c.id for c in cl] == list(range(1, K + 1))


def test_three_cells_meet_in_the_cluster_centre():
    cl = cell.Cluster(1.0, 3)
    want = [-0.5 - 1j * np.sqrt(3) / 2, 1.0, -0.5 + 1j * np.sqrt(3) / 2]
    assert np.max(np.abs(cl.cell_positions - want)) < 1e-15
    assert abs(cl.external_radius - 2.0) < 1e-15
    assert min(np.min(np.abs(c.vertices - cl.pos)) for c in cl) < 1e-15        # the common vertex


def test_wrapped_positions_against_the_reference(fx):
    for i, r in enumerate(fx["geo_radii"]):
        cl = cell.Cluster(float(r), 19)
        assert all(len(p) == 1 for p in cl.wrapped_positions)
        cl.create_wrap_around_cells()
        lists = cl.wrapped_positions
        start = fx["wrap%d_start" % i]
        assert [len(p) for p in lists] == np.diff(start).tolist() and len(lists[0]) == 1
        assert sum(len(p) - 1 for p in lists) == 42 and set(len(p) for p in lists[1:]) == {3, 4}
        assert np.max(np.abs(np.concatenate(lists) - fx["wrap%d_pos" % i])) <= RTOL * 5 * r
        pos, st, ext, centre = cell.hex_tables(19, float(r), True)
        assert np.array_equal(st, start) and np.array_equal(pos, np.concatenate(lists)) and centre == 0
        assert ext == cl.external_radius
        # a wrapped copy lies outside the cluster: farther from the centre than any real cell
        assert min(np.min(np.abs(p[1:])) for p in lists[1:]) > np.max(np.abs(cl.cell_positions))


def test_inside_test_on_chosen_points():
    c = cell.Cell(2.0 + 1.0j, 1.0, 1)
    h = c.height
    inside = [0, 0.99, -0.99, 0.999j * h, 0.49 + 0.99j * h, 0.74 + 0.5j * h * 0.99]
    outside = [1.0, 1.01, 1.001j * h, 0.51 + 0.99j * h, 0.76 + 0.5j * h, -0.76 - 0.5j * h]
    assert all(c.is_point_inside_shape(c.pos + p) for p in inside)
    assert not any(c.is_point_inside_shape(c.pos + p) for p in outside)


# ---- placement ---------------------------------------------------------------------------------------------------------
def test_placement_from_the_stored_uniforms_is_bit_exact(fx):
    """The oracle and cell.py, fed the uniforms the reference consumed, return its positions bit for bit -- the rejected
    candidates included (the attempt counts) -- and consume exactly the stored uniforms."""
    seen_rejection = False
    for c, K, U, ratio, r, S in place_cases(fx):
        uniforms = iter(fx["place%d_uniforms" % c].tolist())
        centres = cell.Cluster(r, K).cell_positions
        for s in range(S):
            want, attempts = fx["place%d_pos" % c][s], fx["place%d_attempts" % c][s]
            used = int(2 * attempts.sum())
            mine = [next(uniforms) for _ in range(used)]
            it = iter(mine)
            for q in range(K * U):
                pos, t, margin = ho.place(centres[q // U], r, ratio, it)
                assert pos == want[q] and t == attempts[q] and margin > ho.EDGE, (c, s, q)
            assert next(it, None) is None
            seen_rejection = seen_rejection or bool(np.any(attempts > 1))
            cl = cell.Cluster(r, K)
            it = iter(mine)
            cl.add_random_users(np.arange(1, K + 1), U, ratio, uniform=lambda: next(it))
            assert np.array_equal(np.array([u.pos for u in cl.get_all_users()]), want) and next(it, None) is None
            assert cl.num_users == K * U and [u.cell_id for u in cl.get_all_users()] == [q // U + 1 for q in range(K * U)]
    assert seen_rejection


def test_distances_and_losses_against_the_reference(fx):
    for c, K, U, ratio, r, S in place_cases(fx):
        cl = cell.Cluster(r, K)
        for s in range(S):
            pos = fx["place%d_pos" % c][s]
            cl.delete_all_users()
            for q, p in enumerate(pos):
                cl.get_cell_by_id(q // U + 1).add_user(cell.Node(p), relative_pos_bool=False)
            assert close(cl.calc_dist_all_users_to_each_cell(), fx["place%d_dist" % c][s])
            assert close([cl.calc_dist(u) for u in cl.get_all_users()], fx["place%d_dcentre" % c][s])
            for name in ("3gpp", "free"):
                if "place%d_pl%s" % (c, name) not in fx:
                    continue
                cfg = ho.base_cfg(K, r, U, ratio, **ho.MODELS[name])
                dist, g = ho.gains(cfg, pos)
                assert close(dist, fx["place%d_dist" % c][s])
                assert close(g[:, :K], fx["place%d_pl%s" % (c, name)][s])
                assert close(g[:, K], fx["place%d_plint%s" % (c, name)][s])
            tx, noise, pe = fx["powers"]
            cfg = ho.base_cfg(K, r, U, ratio, tx=tx, noise=noise, pe=pe)
            d = ho.drop(cfg, pos)
            assert close(d["sinr"], fx["place%d_sinr" % c][s], 1e-12) and close(d["capacity"], fx["place%d_capacity" % c][s], 1e-12)
            op = ho.operator(cfg, pos)
            ok = fx["place%d_assoc_ok" % c][s]
            assert np.array_equal(op["assoc"][ok], fx["place%d_assoc" % c][s][ok])
            assert close(op["sinr"][ok], fx["place%d_sinr_best" % c][s][ok], 1e-12)
    # the library's own host model (what CompSimulator's border loss uses) on the same distances
    model = pathloss.PathLoss3GPP1()
    model.handle_small_distances_bool = True
    assert close(model.calc_path_loss(fx["place1_dist"][0].copy()), fx["place1_pl3gpp"][0])


def test_border_users_against_the_reference(fx):
    grid = cell.Grid()
    grid.create_clusters(1, 3, 1.0)
    cl = grid.get_cluster_from_index(0)
    cl.delete_all_users()
    cl.add_border_users(np.arange(1, 4), np.array([210, -30, 90]), 0.7)
    users = cl.get_all_users()
    assert close([u.pos for u in users], fx["border_app_pos"])
    assert close(cl.calc_dist_all_users_to_each_cell(), fx["border_app_dist"])
    assert close([cl.calc_dist(u) for u in users], fx["border_app_dcentre"])
    # the three users are the farthest points from the cluster centre at 70 % of the way: one figure for all
    assert np.ptp(fx["border_app_dcentre"]) < 1e-12
    for (K, cid, angle, ratio), want in zip(fx["border_more_cfg"], fx["border_more_pos"]):
        cl = cell.Cluster(0.35 if K == 7 else 1.0, int(K))
        cl.add_border_users(int(cid), float(angle), float(ratio))
        got = cl.get_all_users()[0].pos
        assert abs(got - want) <= RTOL * max(abs(want), cl.cell_radius), (K, cid, angle, ratio)
    with pytest.raises(ValueError, match="ratio must be between 0 and 1"):
        cell.Cluster(1.0, 3).add_border_users(1, 30.0, 1.5)
    # an unrotated hexagon has no vertical edge; a cell whose vertices were turned is refused, not divided by zero
    class Turned(cell.Cell):
        vertices = property(lambda self: self.pos + cell.hexagon_vertices(self.radius) * 1j)

    with pytest.raises(NotImplementedError, match="vertical edge"):
        Turned(0j, 1.0, 1).get_border_point(0.0)


# ---- the ledger --------------------------------------------------------------------------------------------------------
def test_ledger_positions_are_disjoint_between_users():
    seen = set()
    for q in range(256):
        pos = ho.ledger_positions(q).reshape(-1).tolist()
        assert len(pos) == 2 * ho.ATTEMPTS and not seen.intersection(pos)
        seen.update(pos)
    assert seen == set(range(2 * 256 * ho.ATTEMPTS)) and max(seen) < 2 ** 32
    assert ho.STREAM_DROP == 5 and ho.ATTEMPTS == cell.MAX_ATTEMPTS
    from oracle import philox
    assert ho.STREAM_DROP not in (philox.STREAM_DATA, philox.STREAM_NOISE, philox.STREAM_CHAN, philox.STREAM_PHASE, 4)


def test_philox_drop_is_a_function_of_seed_and_realization():
    cfg = ho.base_cfg(3, 1.0, 2, 0.7)
    a, fa = ho.philox_drop(cfg, 11, 5)
    b, fb = ho.philox_drop(cfg, 11, 5)
    c, _ = ho.philox_drop(cfg, 11, 6)
    assert np.array_equal(a, b) and fa == fb == 0 and not np.array_equal(a, c)
    centres = cell.Cluster(1.0, 3).cell_positions
    off = a - np.repeat(centres, 2)
    assert all(cell.inside_hexagon(o, 1.0) for o in off) and np.all(np.abs(off) >= 0.7)
    # a ledger of too few attempts flags the drop (the oracle's own rule; on the device 128 attempts never run out)
    pos, t, _ = ho.place(0j, 1.0, 0.0, iter([0.999, 0.999] * 4), max_attempts=4)
    assert pos is None and t == 4


# ---- refused configurations --------------------------------------------------------------------------------------------
def test_what_the_host_geometry_refuses():
    with pytest.raises(RuntimeError, match="Invalid cell type"):
        cell.Cluster(1.0, 3, cell_type="3sec")
    with pytest.raises(RuntimeError, match="Invalid cell type"):
        cell.Cluster(1.0, 3, cell_type="square")
    with pytest.raises(NotImplementedError, match="rotation"):
        cell.Cluster(1.0, 3, rotation=30.0)
    with pytest.raises(ValueError, match="num_cells"):
        cell.Cluster(1.0, 20)
    with pytest.raises(ValueError, match="num_cells"):
        cell.Cluster(1.0, 0)
    with pytest.raises(RuntimeError, match="Wrap around not implemented"):
        cell.Cluster(1.0, 7).create_wrap_around_cells()
    with pytest.raises(ValueError, match="does not implement"):
        cell.Grid().create_clusters(1, 4, 1.0)
    with pytest.raises(NotImplementedError, match="first cluster"):
        cell.Grid().create_clusters(2, 3, 1.0)
    with pytest.raises(ValueError, match="Invalid cell ID"):
        cell.Cluster(1.0, 3).get_cell_by_id(4)
    with pytest.raises(ValueError, match="outside the cell"):
        cell.Cluster(1.0, 3).get_cell_by_id(1).add_user(cell.Node(5.0), relative_pos_bool=False)


def test_abi_surface():
    import ctypes
    assert {"mcle_hex_gains", "mcle_run_hex_drops"} <= set(_lib.exported_symbols())
    assert len(_lib._PROTOS["mcle_hex_gains"][1]) == 9 and len(_lib._PROTOS["mcle_run_hex_drops"][1]) == 15
    assert ctypes.sizeof(_lib.HexCfg) == 8 * 4 + 13 * 8 + 20 * 4 + 2 * 64 * 8


# ---- CompSimulator's argument rules --------------------------------------------------------------------------------------
def test_comp_simulator_argument_rules():
    from pyphysim_amd import simulators
    kw = dict(SNR=[10.0], Pe_dBm=[-10.0], rep_max=4)
    with pytest.raises(ValueError, match="both"):
        simulators.CompSimulator(user_positioning_method="Random", pathloss=np.ones((3, 3)), pathloss_ext=np.ones((3, 1)), **kw)
    with pytest.raises(ValueError, match="both"):
        simulators.CompSimulator(user_positioning_method="Symmetric Far Away", pathloss=lambda f, c: None, **kw)
    with pytest.raises(ValueError, match="user_positioning_method"):
        simulators.CompSimulator(user_positioning_method="Grid", **kw)
    with pytest.raises(ValueError, match="K = 3"):
        simulators.CompSimulator(user_positioning_method="Symmetric Far Away", K=2, **kw)
    with pytest.raises(ValueError, match="cell_radius"):
        simulators.CompSimulator(user_positioning_method="Random", cell_radius=0.0, **kw)
    model = pathloss.PathLoss3GPP1()
    sim = simulators.CompSimulator(user_positioning_method="Random", cell_radius=0.5, **kw)
    assert sim.path_loss_border == model.calc_path_loss(0.5) and sim._pl is None
    far = simulators.CompSimulator(user_positioning_method="Symmetric Far Away", **kw)
    assert far.path_loss_border == model.calc_path_loss(1.0) and far._pl.shape == (3, 3) and far._ple.shape == (3, 1)
    assert simulators.CompSimulator(**kw).path_loss_border == 1.0                   # today's behaviour
