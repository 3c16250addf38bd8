"""Where the step kernel's two new LDS records live (mocca_device.h: L_MID, the per-geom sums of the end points that collide's broad phase
reads; L_LGAP, the gaps of the compacted limit-row candidates): the LDS layout of the three kernel instances restated in numpy, and every
interval that is live together with a new record held against it.  No GPU: index arithmetic, like tests/test_delassus_layout.py.

One wave owns the region [L_V, L_TOTAL) in two views.  A substep runs
    stage joints -> walk (frames; 48 / 64 rows: also S, c, link inertias, bias forces) -> geom points [writes MID] -> collide [reads MID;
    writes the candidate list and the contact records] -> (compact: walk phase 2) -> ABA -> limit compaction [writes ROWD, LGAP] ->
    row build [reads ROWD, LGAP, contacts] -> sweeps [read S / V / 1/D, write the J rows] -> Delassus [X rows, then A] -> PGS -> apply [XL]
so MID is live from the geom points to the end of collide, LGAP from the compaction to the row build."""
import os
import re

import pytest

MAX_PAIRS, MAX_GEOMS = 192, 32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mocca_envs_amd", "csrc", "mocca_device.h")
#        topology: (bodies, geoms, compiled pairs)
TOPOS = {"walker3d": (22, 22, 141), "cassie": (19, 24, 0), "walker2d": (8, 8, 0), "crab2d": (7, 7, 9), "laikago": (13, 32, 0)}


def layout(maxr, compact):
    """float offsets of mocca_device.h's enum for one instance"""
    L = {"V": 216}
    V = L["V"]
    maxc = 20 if maxr >= 64 else (12 if maxr >= 36 else maxr // 3)
    L["B0"], L["SV"], L["SVS"] = V, V + 48, 20
    if compact:
        L["ROWD"] = L["B0"]
        L["CT"] = V + 488
        L["P"] = L["CT"] + 16 * maxc
        L["M"] = L["P"] + 132
        L["RT"] = L["M"]
        L["GP"] = L["M"] + 264
        L["GP_FLOATS"] = 192
        L["CAND"] = L["GP"] + 192
        L["ABA_END"] = L["M"] + 792
        L["A"], L["J"], L["XL"] = V, V + 488, V
        L["MID"] = L["CAND"] + (MAX_PAIRS + 1) // 2
        L["LGAP"] = L["ABA_END"] - maxr
        L["TOTAL"] = max(L["ABA_END"], L["J"] + 28 * (maxr + 1), L["A"] + maxr * maxr)
        L["MID_END_MAX"] = L["ABA_END"]
    else:
        L["A0"], L["GP"], L["CT"] = V + 488, V + 520, V + 656
        L["GP_FLOATS"] = L["CT"] - L["GP"]
        L["ROWD"] = L["CT"] + 16 * maxc
        L["RT"] = L["ROWD"] + 48
        L["M"] = L["RT"] + 264
        L["P"] = L["M"] + 792
        L["ABA_END"] = L["P"] + 132
        L["CAND"] = L["ABA_END"]
        L["A"], L["J"], L["XL"] = V, max(V + 960, L["RT"]), V
        L["MID"] = L["CAND"] + (MAX_PAIRS + 1) // 2
        L["LGAP"] = L["GP"]
        L["TOTAL"] = V + maxr * maxr + 28
        L["MID_END_MAX"] = L["TOTAL"]
    L["MAXR"], L["MAXC"] = maxr, maxc
    return L


INSTANCES = {"r48": layout(48, False), "r32_compact": layout(32, True), "r64": layout(64, False)}


def mid_records(L, topo):
    nb, ng, npair = TOPOS[topo]
    return npair > 0 and 6 * ng <= L["GP_FLOATS"] and L["MID"] + 4 * ng <= L["MID_END_MAX"]


def disjoint(a, b):
    return a[1] <= b[0] or b[1] <= a[0]


def test_the_restated_layout_is_the_products():
    """the numbers mocca_device.h pins with a static_assert of its own, and the two definitions this test restates"""
    L = INSTANCES["r48"]
    assert (L["ROWD"], L["RT"], L["M"], L["P"], L["ABA_END"], L["J"]) == tuple(216 + x for x in (848, 896, 1160, 1952, 2084, 960))
    assert INSTANCES["r32_compact"]["TOTAL"] * 4 <= 8192 and L["TOTAL"] * 4 == 10192 and INSTANCES["r64"]["TOTAL"] * 4 == 17360
    src = open(HEADER).read()
    assert len(re.findall(r"L_MID = L_CAND \+ \(MOCCA_MAX_PAIRS \+ 1\) / 2,", src)) == 2          # both layouts
    assert re.search(r"L_LGAP = L_ABA_END - MAXR,", src) and re.search(r"L_LGAP = L_GP,", src)
    assert re.search(r"MID_RECORDS = T::NPAIR > 0 && 6 \* T::NG <= GP_FLOATS && L_MID \+ 4 \* T::NG <= \(COMPACT \? \(int\)L_ABA_END : \(int\)L_TOTAL\)", src)
    for name, (nb, ng, npair) in TOPOS.items():
        t = open(os.path.join(os.path.dirname(HEADER), f"topo_{name}.h")).read()
        assert re.search(rf"NB = {nb};", t) and re.search(rf"NG = {ng};", t) and re.search(rf"NPAIR = {npair};", t), name


@pytest.mark.parametrize("inst,topo", [(i, t) for i in INSTANCES for t in TOPOS if (i, t) != ("r32_compact", "cassie")])   # closure topologies have no compact instance
def test_midpoint_records(inst, topo):
    L = INSTANCES[inst]
    nb, ng, npair = TOPOS[topo]
    if topo == "walker3d":
        assert mid_records(L, topo), "the headline topology must take the trimmed broad phase in every instance"
    if not mid_records(L, topo):
        return                                                  # keeps the broad phase that reads the geom points
    mid = (L["MID"], L["MID"] + 4 * ng)
    assert L["MID"] % 4 == 0 and mid[1] <= L["TOTAL"]           # 16-byte records inside the wave's LDS
    live = {"persistent state": (0, L["V"]),
            "geom points": (L["GP"], L["GP"] + 6 * ng),          # written by the same lanes, read by both collision passes
            "candidate list": (L["CAND"], L["CAND"] + (MAX_PAIRS + 1) // 2),
            "contact records": (L["CT"], L["CT"] + 16 * L["MAXC"]),
            "body frames": (L["RT"], L["RT"] + 12 * 22)}          # geom_points reads them; compact: walk phase 2 reads them after collide
    if not inst.endswith("compact"):                             # 48 / 64 rows: the walk has already left S, c, link inertias and bias forces for the ABA
        live["body records"] = (L["SV"], L["SV"] + 22 * L["SVS"])
        live["link inertias"] = (L["M"], L["M"] + 36 * 22)
        live["bias forces"] = (L["P"], L["P"] + 6 * 22)
    else:                                                         # compact: the joint records of the walk's second phase
        live["joint records"] = (L["SV"], L["SV"] + 22 * L["SVS"])
        assert mid[1] <= L["ABA_END"]                             # under the link inertias phase 2 writes AFTER collide
    for what, iv in live.items():
        assert disjoint(mid, iv), (inst, topo, what, mid, iv)


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_limit_gaps(inst):
    L = INSTANCES[inst]
    gaps = (L["LGAP"], L["LGAP"] + L["MAXR"])                     # one float per compacted candidate, rank < max_rows <= MAXR
    assert gaps[1] <= L["TOTAL"]
    live = {"persistent state": (0, L["V"]),
            "candidates": (L["ROWD"], L["ROWD"] + 48),
            "body records (S, V, 1/D)": (L["SV"], L["SV"] + 22 * L["SVS"]),
            "contact records": (L["CT"], L["CT"] + 16 * L["MAXC"]),
            # the sweeps' J rows (+ the dummy row) are written by lanes that may run ahead of nothing: one wave, program order -- but a
            # limit row's lane reads its gap BEFORE its first J store only if the two never share an address
            "J rows": (L["J"], L["J"] + 28 * (L["MAXR"] + 1))}
    if not inst.endswith("compact"):
        live["body frames (closure rows)"] = (L["RT"], L["RT"] + 12 * 22)
    for what, iv in live.items():
        assert disjoint(gaps, iv), (inst, what, gaps, iv)
    # what the gaps overwrite is dead at the compaction: the geom points (48 / 64 rows; the observation is assembled there only after the
    # last substep), the last body's link inertia (compact: the ABA is over)
    if inst.endswith("compact"):
        assert L["M"] <= gaps[0] and gaps[1] <= L["M"] + 36 * 22
    else:
        assert L["GP"] <= gaps[0] and gaps[1] <= L["GP"] + L["GP_FLOATS"]
