"""Mirror tables over a row that ends in the observation-action history (symmetry.mirror_tables(history=)): the extended tables are an
involution; they are equivariant with the history rule in pure numpy -- the mirror of the restated row of a sequence is the restated row of
the mirrored sequence, bit for bit; a column set that is not closed under the mirror is refused by name; without `history=` nothing
changes."""
import numpy as np
import pytest

import history_reference as R
from mocca_envs_amd import host_logic as H, model as M
from mocca_envs_amd.perception import scan_grid
from mocca_envs_amd.symmetry import check_tables, mirror_tables

OBS, ACT = 52, 21


@pytest.fixture(scope="module")
def mi():
    return H.mirror_indices(M.compile_walker3d(), stepper=False)


def closed_columns(mi, seed, count):
    """`count` columns and their mirror images, in a shuffled order"""
    perm = mirror_tables(mi, OBS, ACT)[0]
    rng = np.random.default_rng(seed)
    pick = rng.choice(OBS, count, replace=False)
    cols = np.unique(np.concatenate([pick, perm[pick]]))
    return [int(c) for c in rng.permutation(cols)]


def configs(mi):
    return [(3, 1, list(range(OBS)), ACT), (2, 3, closed_columns(mi, 1, 5), ACT), (4, 2, [], ACT), (16, 1, [0], 0), (2, 1, closed_columns(mi, 2, 9), 0)]


def test_without_a_history_the_tables_are_what_they_were(mi):
    pts = scan_grid((0.0, 0.5), (-0.25, 0.25), 3, 4)
    for kw in (dict(), dict(scan_points=pts), dict(depth_shape=(3, 5)), dict(scan_points=pts, depth_shape=(3, 5))):
        plain, none = mirror_tables(mi, OBS, ACT, **kw), mirror_tables(mi, OBS, ACT, history=None, **kw)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(plain, none))
        ext = mirror_tables(mi, OBS, ACT, history=(list(range(OBS)), ACT, 2), **kw)      # the head of the extended tables is the plain table
        n = len(plain[0])
        assert np.array_equal(ext[0][:n], plain[0]) and np.array_equal(ext[1][:n], plain[1])
        assert np.array_equal(ext[2], plain[2]) and np.array_equal(ext[3], plain[3]) and len(ext[0]) == n + 2 * (OBS + ACT)


def test_extended_tables_are_an_involution_that_stays_inside_each_pair(mi):
    for K, s, cols, A in configs(mi):
        in_perm, in_sign, act_perm, act_sign = mirror_tables(mi, OBS, ACT, history=(cols, A, K))
        W = len(cols) + A
        assert len(in_perm) == OBS + K * W
        check_tables((in_perm, in_sign, act_perm, act_sign), in_dim=OBS + K * W, act_dim=ACT)
        assert np.array_equal(in_perm[in_perm], np.arange(len(in_perm))) and np.array_equal(in_sign[in_perm], in_sign)
        for j in range(K):
            lo = OBS + j * W
            block = in_perm[lo:lo + W] - lo
            assert block.min() >= 0 and block.max() < W                      # a pair mirrors into itself
            for p, c in enumerate(cols):                                     # observation entry p: where in_perm[c] sits, with c's sign
                assert cols[block[p]] == in_perm[c] and in_sign[lo + p] == in_sign[c]
            if A:
                assert np.array_equal(block[len(cols):] - len(cols), act_perm) and np.array_equal(in_sign[lo + len(cols):lo + W], act_sign)


def test_mirror_equivariance_with_the_rule_in_numpy(mi):
    """M row(sequence) == row(M sequence), on bits: a random sequence with an episode boundary and a call without an action"""
    n, calls = 5, 24
    rng = np.random.default_rng(5)
    obs_perm, obs_sign, act_perm, act_sign = mirror_tables(mi, OBS, ACT)
    for K, s, cols, A in configs(mi):
        in_perm, in_sign, _, _ = mirror_tables(mi, OBS, ACT, history=(cols, A, K))
        plain, mirrored = R.History(n, K, s, cols, A), R.History(n, K, s, cols, A)
        t, e, full = np.zeros(n, np.int64), np.zeros(n, np.int64), 0
        for k in range(calls):
            obs = rng.standard_normal((n, OBS)).astype(np.float32)
            act = None if k in (0, 13) else rng.standard_normal((n, ACT)).astype(np.float32)
            row = np.concatenate([obs, plain(obs, act, t, e)], 1)
            m_obs = obs[:, obs_perm] * obs_sign
            m_act = None if act is None else act[:, act_perm] * act_sign
            m_row = np.concatenate([m_obs, mirrored(m_obs, m_act, t, e)], 1)
            # on bits, but for the sign of a zero: the mirror's sign flip turns the +0.0 of an empty pair into -0.0 (x + 0.0 undoes that alone)
            assert np.array_equal((row[:, in_perm] * in_sign + np.float32(0.0)).view(np.uint32), (m_row + np.float32(0.0)).view(np.uint32)), (K, s, k)
            full += int((row[:, OBS:] != 0).any())
            t += 1
            ended = (k == 17) & (np.arange(n) % 2 == 0)
            t[ended], e[ended] = 0, e[ended] + 1
        assert full > calls // 2


def test_a_column_set_that_is_not_closed_is_refused_by_name(mi):
    perm = mirror_tables(mi, OBS, ACT)[0]
    c = int(np.flatnonzero(perm != np.arange(OBS))[0])          # a column that swaps with another
    with pytest.raises(ValueError, match=rf"history column {c} mirrors to column {int(perm[c])}"):
        mirror_tables(mi, OBS, ACT, history=([c], ACT, 2))
    mirror_tables(mi, OBS, ACT, history=([c, int(perm[c])], ACT, 2))
    with pytest.raises(ValueError, match="0 or the policy's act_dim"):
        mirror_tables(mi, OBS, ACT, history=([0], 15, 2))
    with pytest.raises(ValueError, match="history column 52 is outside"):
        mirror_tables(mi, OBS, ACT, history=([52], 0, 2))
