"""The lane layout of the kinematics walk's second phase where it forms the body velocities level by level (mocca_device.h walk_phase2,
WALK_LEVELS): the lanes are the ABA outward pass's (csrc/topo_*.h out_body, the top bits of kLanePk), a lane takes what the lane on its
LEFT holds, and the base sits on the last lane without a body.  The tables are the whole correctness argument of the data flow, so the
rounds are run here on symbols, for every generated header with OUTWARD_DPP, exactly as the kernel runs them:

  * a lane's value is the ordered tuple of the joints folded into it; every lane starts from the base's (the empty tuple);
  * MAXD - 1 times: link = value + (own joint,), then value = the left neighbour's link -- but a row's first lane has no source and keeps
    what it has, and only lanes with a body take part (the others are masked out, and no lane may read one of them);
  * the body's velocity is value + (own joint,), and value the parent's.

After that every body's tuple must be its root->body path in model.py's tree, the same on both lanes of a body that two rows host, and
exactly one lane per body -- the base included -- must be the storing one."""
import pytest

from mocca_envs_amd import model as M
from test_outward_layout import ROW, TOPOLOGIES, _header

WITH_LEVELS = [name for name in TOPOLOGIES if _header(name)["dpp"]]


def _path(parent, b):
    p = []
    while b > 0:
        p.append(b)
        b = parent[b]
    return tuple(p[::-1])


def _run_rounds(lane_bits, maxd):
    """-> (parent's tuple, body's tuple) per lane, None on the lanes without a body"""
    body = [w & 31 for w in lane_bits]
    active = [b != 0 for b in body]
    t = [()] * 64
    for _ in range(1, maxd):
        link = [t[l] + (body[l],) for l in range(64)]
        for l in range(64):
            if active[l] and l % ROW != 0:       # row_shr:1 without bound_ctrl: the first lane of a row is not written
                assert active[l - 1], ("a lane with a body reads a masked lane", l)
                t[l] = link[l - 1]
    return [(t[l], t[l] + (body[l],)) if active[l] else None for l in range(64)]


def test_some_topology_takes_the_levels():
    assert "Walker3D" in WITH_LEVELS and "Cassie" not in WITH_LEVELS


@pytest.mark.parametrize("name", WITH_LEVELS)
def test_rounds_fold_the_root_to_body_path(name):
    h = _header(name)
    m = TOPOLOGIES[name][1]()
    nb = m.n_bodies
    parent = [m.parent[b] for b in range(nb)]
    lane_bits = [w >> M.OUTWARD_SHIFT for w in h["lane_pk"]]
    assert [w & 31 for w in lane_bits] == [max(b, 0) for b in h["out_body"]]      # what the kernel reads is what the table says
    assert h["maxd"] == max(m.depth[b] for b in range(nb))
    got = _run_rounds(lane_bits, h["maxd"])
    seen = {}
    for l, g in enumerate(got):
        if g is None:
            assert h["out_body"][l] < 0
            continue
        b = h["out_body"][l]
        assert g[1] == _path(parent, b), ("body's joints, in order", l, b, g[1])
        assert g[0] == _path(parent, parent[b]), ("parent's joints", l, b, g[0])
        assert seen.setdefault(b, g) == g, ("a body on two rows gets two values", b)
    assert sorted(seen) == list(range(1, nb))


@pytest.mark.parametrize("name", WITH_LEVELS)
def test_one_storing_lane_per_body(name):
    h = _header(name)
    nb = len(h["parent"])
    lane_bits = [w >> M.OUTWARD_SHIFT for w in h["lane_pk"]]
    idle = [l for l in range(64) if h["out_body"][l] < 0]
    assert idle, "the base needs a lane without a body"
    base_lane = idle[-1]                                  # walk_base_lane(): the last lane without a body
    stores = [lane_bits[l] & 31 if 1 <= lane_bits[l] < 32 else 0 if l == base_lane else None for l in range(64)]
    assert lane_bits[base_lane] == 0, "the base's lane runs body 0"
    for b in range(nb):
        assert stores.count(b) == 1, ("storing lanes of body", b)
    # a lane that stores hosts the body it stores
    assert all(s is None or s == max(h["out_body"][l], 0) for l, s in enumerate(stores))
    # the base's lane is no lane a chain reads: a chain's lanes read only chain lanes (checked above), and it lies behind its row's chain
    row = h["out_body"][ROW * (base_lane // ROW):ROW * (base_lane // ROW + 1)]
    assert all(b < 0 for b in row[base_lane % ROW:])
