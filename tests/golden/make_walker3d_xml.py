#!/usr/bin/env python3
"""The numbers of the reference's data/robots/walker3d.xml that the model compiler uses, as a data fixture
(tests/test_model.py::test_table_matches_reference_xml compares the compiled table against it): per body its parent, pos and
quat; per joint its name, axis, range and pos; per geom its name, type, size, fromto / pos, contype and conaffinity; and the
<default> joint armature and damping and geom friction.  Numbers and names only, in file order.
Output: tests/golden/walker3d_xml.json.
Re-run:  python tests/golden/make_walker3d_xml.py <reference checkout>/mocca_envs/data/robots/walker3d.xml
"""
from __future__ import annotations

import json
import os
import sys
import xml.etree.ElementTree as ET

HERE = os.path.dirname(os.path.abspath(__file__))


def nums(s):
    return None if s is None else [float(x) for x in s.split()]


def main(xml_path: str) -> None:
    root = ET.parse(xml_path).getroot()
    bodies = []

    def rec(b, parent):
        bodies.append({
            "name": b.get("name"), "parent": parent, "pos": nums(b.get("pos")), "quat": nums(b.get("quat")),
            "joints": [{"name": j.get("name"), "axis": nums(j.get("axis")), "range": nums(j.get("range")), "pos": nums(j.get("pos"))}
                       for j in b.findall("joint")],
            "geoms": [{"name": g.get("name"), "type": g.get("type"), "size": nums(g.get("size")), "fromto": nums(g.get("fromto")),
                       "pos": nums(g.get("pos")), "contype": int(g.get("contype", 3)), "conaffinity": int(g.get("conaffinity", 3))}
                      for g in b.findall("geom")],
        })
        for ch in b.findall("body"):
            rec(ch, b.get("name"))
    rec(root.find("worldbody").find("body"), None)
    d = root.find("default")
    out = {"bodies": bodies, "default_joint": {"armature": float(d.find("joint").get("armature")), "damping": float(d.find("joint").get("damping"))},
           "default_geom": {"friction": nums(d.find("geom").get("friction"))}}
    path = os.path.join(HERE, "walker3d_xml.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, len(bodies), "bodies")


if __name__ == "__main__":
    main(sys.argv[1])
