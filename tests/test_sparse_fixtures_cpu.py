"""The fixtures of the sparse conformance suite (tests/sparse_fixtures.py) reach the edges their case ids name -- checked on the
CPU with oracle_np.sparse_conv_rules, so a fixture that drifts is caught without a GPU."""
import numpy as np

from tests import sparse_fixtures as F


def test_dense_fixture_has_full_slots_of_27_taps():
    g = F.dense()
    out_idx, _, nbr = g.rules("subm")
    assert np.array_equal(out_idx, g.idx)
    for sites in (64, 128):
        full = F.full_slots(nbr, sites)
        assert full.size >= 1, f"no {sites}-site slot with 27 live taps at every site"
    # such a slot is the worst case of the pair tiles: 27 taps x 4 whole tiles of 16 pairs = 108 tiles
    s = int(F.full_slots(nbr)[0])
    live = (nbr[s * 64:(s + 1) * 64] >= 0).sum(0)
    assert int(((live + 15) // 16).sum()) == 108
    for layer in ("s2", "s2p011"):
        assert (g.rules(layer)[2] >= 0).sum(1).max() == 27


def test_isolated_fixture_has_only_centre_taps():
    g = F.isolated()
    _, _, nbr = g.rules("subm")
    assert np.array_equal(nbr[:, 13], np.arange(g.n))
    assert ((nbr >= 0).sum(1) == 1).all()


def test_faces_fixture_has_out_of_grid_taps_on_every_side():
    g = F.faces()
    lo, hi = g.idx[:, 1:].min(0), g.idx[:, 1:].max(0)
    assert (lo == 0).all() and np.array_equal(hi, np.array(g.shape) - 1)
    assert all(s % 2 == 1 for s in g.shape)
    for layer in ("s2", "s2p011"):
        out_idx, out_shape, nbr = g.rules(layer)
        ks, st, pd, _ = F.LAYERS[layer]
        c = out_idx[:, None, 1:].astype(np.int64) * st - pd + np.stack(np.meshgrid(*(np.arange(k) for k in ks), indexing="ij"), -1).reshape(1, -1, 3)
        outside = ((c < 0) | (c >= np.array(g.shape))).any(2)
        assert (nbr[outside] == -1).all()
        for d in range(3):              # a tap below 0 and a tap past the end in every dimension
            assert (c[..., d] < 0).any() == (pd[d] > 0) and (c[..., d] >= g.shape[d]).any() == (g.shape[d] % 2 == 1 and pd[d] > 0)


def test_seam_fixture_has_adjacent_sites_across_batches_and_no_crossing_pair():
    g = F.seam()
    k = F.keys(g.idx, g.shape)
    sk = F.seam_keys(g.shape, g.batch)
    assert np.isin(sk, k).all() and (np.diff(sk.reshape(-1, 2), axis=1) == 1).all()
    for layer in ("subm", "s2", "s2p011"):
        out_idx, _, nbr = g.rules(layer)
        o, t = np.nonzero(nbr >= 0)
        assert np.array_equal(g.idx[nbr[o, t], 0], out_idx[o, 0])
    # the two sites at a seam are neighbours in key order but not in space: neither sees the other
    _, _, nbr = g.rules("subm")
    rows = np.searchsorted(k, sk)
    for a, b in rows.reshape(-1, 2):
        assert b not in nbr[a] and a not in nbr[b]


def test_count_fixtures_have_their_site_counts():
    for n in F.COUNTS:
        g = F.counts(n)
        assert g.n == n and g.batch == 1


def test_largest_fixtures_stay_exact_in_fp32():
    rng = np.random.default_rng(0)
    g = F.dense()
    for layer, cin, cout in (("subm", 128, 64), ("s2", 64, 128)):
        _, _, nbr = g.rules(layer)
        x = F.features(rng, g.n, cin)
        w = F.weights(rng, nbr.shape[1], cin, cout)
        sc, sh = F.batchnorm(rng, cout)
        _, bound = F.conv_ref(x, nbr, w)
        assert F.bn_bound(bound, sc, sh).max() < F.EXACT
    nbr = F.wgrad_table(rng, 4097, 3000, 27, density=1.0)
    x, g_ = F.features(rng, 3000, 64), F.features(rng, 4097, 64)
    part, bound = F.wgrad_ref(x, g_, nbr)
    assert part.shape == (3, 27, 64, 64) and bound.max() < F.EXACT


def test_wgrad_table_hits_stage_seams():
    rng = np.random.default_rng(1)
    for n_out in (2047, 2048, 2049, 4097):
        nbr = F.wgrad_table(rng, n_out, 500, 27)
        assert [(nbr[:2048, t] >= 0).sum() for t in range(3)] == [31, 32, 33]
        assert (nbr[-1] >= 0).all() and (nbr[min(n_out, 2048) - 1, :3] >= 0).all()
