"""The compile-time child table of every generated topology header (mocca_envs_amd/csrc/topo_*.h: `cchild`) is what the constraint
rows' outward sweep decides by which bodies have no children (mocca_device.h has_child: such a body's acceleration and joint motion
vector are not formed).  Read as text, it must agree row for row with the runtime table `kChild*`, and a body must be childless in it
exactly when no body names it as `parent`.  No GPU."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mocca_envs_amd", "csrc")
HEADERS = sorted(glob.glob(os.path.join(CSRC, "topo_*.h")))


def _ints(text):
    return [int(x) for x in re.findall(r"-?\d+", text)]


def _rows(body):
    """'{{4, 1}, {2, -1}}' or the multi-line form -> [[4, 1], [2, -1]]"""
    return [_ints(r) for r in re.findall(r"\{([^{}]*)\}", body)]


def _tables(path):
    src = open(path).read()
    m = re.search(r"kChild\w+\[(\d+)\]\[(\d+)\]\s*=\s*\{(.*?)\n\};", src, re.S)
    assert m, "no kChild table"
    nb, maxch, kchild = int(m.group(1)), int(m.group(2)), _rows(m.group(3))
    m = re.search(r"static constexpr int cchild\(int b, int k\) \{ constexpr int t\[(\d+)\]\[(\d+)\] = \{(.*?)\}; return b < 0 \? -1 : t\[b\]\[k\]; \}", src)
    assert m, "no cchild table"
    cdims, cchild = (int(m.group(1)), int(m.group(2))), _rows(m.group(3))
    m = re.search(r"static constexpr int parent\(int b\) \{ constexpr int t\[(\d+)\] = \{(.*?)\};", src)
    assert m, "no parent table"
    parent = _ints(m.group(2))
    assert int(m.group(1)) == len(parent)
    consts = {k: int(v) for k, v in re.findall(r"static constexpr int (NB|MAXCH) = (\d+);", src)}
    return nb, maxch, kchild, cdims, cchild, parent, consts


def test_every_topology_header_is_read():
    assert {os.path.basename(h) for h in HEADERS} >= {"topo_walker3d.h", "topo_cassie.h", "topo_walker2d.h", "topo_crab2d.h", "topo_laikago.h"}


@pytest.mark.parametrize("path", HEADERS, ids=[os.path.basename(h) for h in HEADERS])
def test_cchild_is_the_child_table(path):
    nb, maxch, kchild, cdims, cchild, parent, consts = _tables(path)
    assert consts == {"NB": nb, "MAXCH": maxch} and cdims == (nb, maxch) and len(parent) == nb
    assert len(kchild) == nb and len(cchild) == nb and all(len(r) == maxch for r in kchild + cchild)
    for b in range(nb):
        assert cchild[b] == kchild[b], (b, cchild[b], kchild[b])
        kids = [c for c in cchild[b] if c >= 0]
        assert sorted(kids) == sorted(c for c in range(nb) if parent[c] == b), (b, kids)     # the row holds the body's children, each once
        assert all(c == -1 for c in cchild[b] if c < 0)
    named = {p for p in parent if p >= 0}
    for b in range(nb):
        childless = all(c < 0 for c in cchild[b])
        assert childless == (b not in named), (b, cchild[b])
    assert parent[0] == -1 and all(0 <= parent[b] < b for b in range(1, nb))     # the sweeps visit a parent before its children


def test_the_walkers_leaves():
    nb, _, _, _, cchild, _, _ = _tables(os.path.join(CSRC, "topo_walker3d.h"))
    assert [b for b in range(nb) if all(c < 0 for c in cchild[b])] == [8, 13, 17, 21]
