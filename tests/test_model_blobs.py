"""Byte-for-byte pin of every model blob the compiler writes (tests/golden/model_blobs.npz).

The blob is the one input the HIP kernels, the f32/f64 oracle and the fuzz generator share; a change of the compiler that is meant to
leave the physics alone must leave these bytes alone.  `python tests/test_model_blobs.py` rewrites the fixture from the current tree;
pytest only compares."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mocca_envs_amd import model as M          # noqa: E402
from mocca_envs_amd import pybullet_dump as PD  # noqa: E402
from mocca_envs_amd import vec_env             # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "model_blobs.npz")


def _hand_tree():
    """A small MJCF-style tree that reaches the compiler options no shipped robot combines: a non-unit hinge axis, a two-hinge body,
    a hinge-less child merged into its parent, a torso link, a forced link mass, a tilted start and self collision."""
    G, B, H = M.Geom, M.Body, M.Hinge
    foot = B("foot", (0.0, 0.0, -0.3), anchor=(0.0, 0.0, 0.02), hinges=[H("ankle", (0.0, 2.0, 0.5), -30, 40, 25)],
             geoms=[G("sole", M.GEOM_CAPSULE, 0.04, (-0.05, 0.0, 0.0), (0.12, 0.0, 0.0), friction=0.9)])
    shin = B("shin", (0.0, 0.1, -0.1), anchor=(0.0, 0.0, 0.05), quat_wxyz=(0.99, 0.05, 0.0, 0.1),
             hinges=[H("hip_x", (1.0, 0.0, 0.0), -20, 20, 50), H("hip_y", (0.0, 1.0, 0.0), -90, 30, 70)],
             geoms=[G("shin", M.GEOM_CAPSULE, 0.05, (0.0, 0.0, 0.0), (0.0, 0.0, -0.28))], children=[foot])
    knob = B("knob", (0.0, -0.05, 0.02), geoms=[G("knob", M.GEOM_SPHERE, 0.03, (0.0, 0.0, 0.0), group=1, mask=1)])
    arm = B("arm", (0.1, -0.15, 0.1), hinges=[H("shoulder", (0.0, 0.0, 1.0), -45, 60, 30)],
            geoms=[G("arm", M.GEOM_CAPSULE, 0.03, (0.0, 0.0, 0.0), (0.0, -0.2, 0.0))], children=[knob])
    return B("root", (0.0, 0.0, 1.0), geoms=[G("core", M.GEOM_SPHERE, 0.12, (0.0, 0.0, 0.0)),
                                             G("belly", M.GEOM_SPHERE, 0.08, (0.0, 0.0, -0.1), group=2, mask=2)],
             children=[shin, arm])


def _dump_round_trip(tm, joint_names, **kw):
    return PD.from_pybullet_dump(PD.synthetic_dump(tm, joint_names, **kw), tm, joint_names)


def _str_bytes(names):
    return "\n".join(names).encode()


def variants():
    """{name: bytes}: every blob variant the pin covers."""
    out = {}
    for env_id in sorted(vec_env.TASKS):
        out["env:" + env_id] = vec_env.compile_model_for(env_id).to_bytes()
    for pc in sorted(M.PLANK_CLASSES):
        out["walker3d_stepper:" + pc] = M.compile_walker3d(M.TASK_WALKER3D_STEPPER, plank_class=pc).to_bytes()
        out["mike_stepper:" + pc] = M.compile_mike(plank_class=pc).to_bytes()
        out["laikago_stepper:" + pc] = M.compile_laikago(stepper=True, plank_class=pc).to_bytes()
    for planar in (False, True):
        for mode in (M.CASSIE_PLAIN, M.CASSIE_PHASE_MOCCA, M.CASSIE_PHASE_MIRROR):
            for rsi in (False, True):
                for rc in (False, True):
                    out[f"cassie:planar{int(planar)}_mode{mode}_rsi{int(rsi)}_rc{int(rc)}"] = M.compile_cassie(
                        planar=planar, power_coef=0.7, residual_control=rc, mode=mode, rsi=rsi).to_bytes()
    out["bullet_fidelity:walker3d"] = M.bullet_fidelity(M.compile_walker3d()).to_bytes()
    from mocca_envs_amd.mjcf_tables import mike_description
    out["compile_model:mike_raw"] = M.compile_model(mike_description(), ["right_foot", "left_foot"], {}, (0, 0, 1), [], [], []).to_bytes()
    out["compile_model:hand_tree"] = M.compile_model(
        _hand_tree(), ["foot"], {"hip_y": -0.3, "ankle": 0.2}, (0.1, -0.2, 1.1), [1], [3], [0],
        joint_damping=0.3, joint_armature=0.02, self_collision=True, init_quat_xyzw=(0.0, 0.1, 0.0, 0.995),
        link_mass={"hip_y": 3.5}, torso_name="arm").to_bytes()
    out["dump:walker3d"] = _dump_round_trip(M.compile_walker3d(), M.WALKER3D_JOINT_NAMES, fixed_children={2: 0.25}, base_axes_aligned=True,
                                            link_names=M.WALKER3D_LINK_NAMES).to_bytes()
    jn, ln = M.cassie_joint_names()
    out["dump:cassie"] = _dump_round_trip(M.compile_cassie(), jn, fixed_children={3: 0.2}, base_axes_aligned=True, all_axes_aligned=True,
                                          link_names=ln, fixed_prefix="fixed_extra_").to_bytes()
    tl = M.compile_laikago()
    toes = {int(tl.foot_body[f]): M.LAIKAGO_FEET[f] for f in range(4)}
    out["dump:laikago"] = _dump_round_trip(tl, M.LAIKAGO_JOINTS, fixed_children={b: 0.02 for b in toes}, base_axes_aligned=True,
                                           fixed_prefix="jtoe_", link_names=[n.split("_2_")[0] for n in M.LAIKAGO_JOINTS],
                                           fixed_link_names=toes).to_bytes()
    out["names:cassie_joints"] = _str_bytes(jn)
    out["names:cassie_links"] = _str_bytes(ln)
    return out


def _first_field_diff(a: bytes, b: bytes) -> str:
    if len(a) != len(b):
        return f"length {len(a)} != {len(b)}"
    ma, mb = M.MoccaModel.from_buffer_copy(a), M.MoccaModel.from_buffer_copy(b)
    for name, _ in M.MoccaModel._fields_:
        off, size = getattr(M.MoccaModel, name).offset, getattr(M.MoccaModel, name).size
        if a[off:off + size] != b[off:off + size]:
            return f"field {name!r}: {np.array(getattr(ma, name)).tolist()} != {np.array(getattr(mb, name)).tolist()}"
    return "no field differs"


def test_blobs_are_byte_identical():
    with np.load(FIXTURE) as z:
        pinned = {k: z[k].tobytes() for k in z.files}
    current = variants()
    assert sorted(current) == sorted(pinned)
    bad = []
    for name in sorted(pinned):
        got, want = current[name], pinned[name]
        if got == want:
            continue
        if name.startswith("names:"):
            bad.append(f"{name}: {got.decode().split()} != {want.decode().split()}")
        else:
            bad.append(f"{name}: first difference in {_first_field_diff(got, want)}")
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    blobs = variants()
    np.savez_compressed(FIXTURE, **{k: np.frombuffer(v, np.uint8) for k, v in blobs.items()})
    print(f"wrote {len(blobs)} variants to {os.path.relpath(FIXTURE, ROOT)}")
