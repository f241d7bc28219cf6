"""The joints' records and declarations without a GPU (include/nudge_hip.h, "joints"): sizes and offsets from gcc against the ctypes and numpy mirrors of
nudge_amd/engine.py, the four declarations present, exported and wrapped, and the header's "Not built" line."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostjoint_util as HJ                  # noqa: E402
from nudge_amd import engine as E           # noqa: E402

CALLS = ("nh_joints_prepare", "nh_joints_setup", "nh_joints_apply", "nh_joint_connections")


def test_the_calls_are_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int nh_joints_prepare(nh_context* ctx, uint32_t bodies_count, const nh_JointList* list, const nh_JointPlan* plan);" in flat
    assert ("int nh_joints_setup(nh_context* ctx, const nh_ActiveBodies* active_bodies, const nh_BodyData* bodies, const nh_JointList* list, "
            "const nh_JointPlan* plan, const nh_JointParams* params, const nh_JointImpulse* impulses);") in flat
    assert ("int nh_joints_apply(nh_context* ctx, const nh_BodyData* bodies, const nh_JointList* list, const nh_JointPlan* plan, nh_JointImpulse* impulses, "
            "uint32_t iterations);") in flat
    assert "int nh_joint_connections(nh_context* ctx, const nh_JointList* list, nh_BodyPair* out);" in flat
    syms = subprocess.check_output(["nm", "-D", "--defined-only", E._LIB_PATH], text=True)
    for name in CALLS:
        assert name in E.EXPORTS
        assert re.search(r"\bT %s$" % name, syms, flags=re.M), name
        assert hasattr(E.lib(), name)
    for name in ("joints_prepare", "joints_setup", "joints_apply", "step_joints", "joint_status"):
        assert callable(getattr(E.World, name))
    text = re.sub(r"\s+", " ", hdr)
    for line in ("weld joints", "hinge limits and motors", "springs", "block (3x3) solves", "assemblies over 1024 joints", "joints inside nh_step and still steps",
                 "partitioned worlds", "`namespace nudge` extension", "NOT MEASURED YET (tools/joints.py", "joints can only FOLLOW it",
                 "j_owner", "j_levels", "j_setup", "j_sweep", "j_connections"):
        assert line in text, line
    note9 = [line for line in hdr.splitlines() if "nh_joints_setup and nh_joints_apply ARE entry points of the step" in line]
    assert len(note9) == 1


def test_records_are_the_headers(tmp_path):
    probes = [("nh_Joint", "a", E.Joint, E.JOINT), ("nh_Joint", "flags", E.Joint, E.JOINT), ("nh_Joint", "anchor_a", E.Joint, E.JOINT),
              ("nh_Joint", "anchor_b", E.Joint, E.JOINT), ("nh_Joint", "p", E.Joint, E.JOINT),
              ("nh_JointImpulse", "row", E.JointImpulse, E.JOINT_IMPULSE), ("nh_JointImpulse", "reserved", E.JointImpulse, E.JOINT_IMPULSE),
              ("nh_JointParams", "baumgarte", E.JointParams, None), ("nh_JointParams", "warm", E.JointParams, None),
              ("nh_JointList", "offsets", E.JointList, None), ("nh_JointList", "count", E.JointList, None), ("nh_JointList", "assemblies", E.JointList, None),
              ("nh_JointPlan", "levels", E.JointPlan, None), ("nh_JointPlan", "order", E.JointPlan, None), ("nh_JointPlan", "capacity", E.JointPlan, None),
              ("nh_JointPlan", "reserved", E.JointPlan, None)]
    body = "".join(f'  printf("%zu %zu\\n", sizeof({c}), offsetof({c}, {m}));\n' for c, m, _, _ in probes)
    body += ('  printf("%u %u %u %u %u %u %u %u\\n", (unsigned)NH_JOINT_BALL, (unsigned)NH_JOINT_DISTANCE, (unsigned)NH_JOINT_HINGE, (unsigned)NH_JOINT_BIN, '
             '(unsigned)NH_JOINT_ASSEMBLY_MAX, (unsigned)NH_JOINT_ERR_ASSEMBLY_SIZE, (unsigned)NH_JOINT_ERR_SHARED_BODY, (unsigned)NH_JOINT_ERR_OFFSETS);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for (c, m, mirror, dtype), line in zip(probes, lines):
        size, off = (int(x) for x in line.split())
        assert (size, off) == (C.sizeof(mirror), getattr(mirror, m).offset), (c, m, size, off)
        if dtype is not None:
            assert (size, off) == (dtype.itemsize, dtype.fields[m][1]), (c, m, size, off)
    assert [int(x) for x in lines[len(probes)].split()] == [E.NH_JOINT_BALL, E.NH_JOINT_DISTANCE, E.NH_JOINT_HINGE, E.NH_JOINT_BIN, E.NH_JOINT_ASSEMBLY_MAX,
                                                            E.NH_JOINT_ERR_ASSEMBLY_SIZE, E.NH_JOINT_ERR_SHARED_BODY, E.NH_JOINT_ERR_OFFSETS]
    assert (C.sizeof(E.Joint), C.sizeof(E.JointImpulse), C.sizeof(E.JointParams)) == (64, 32, 16)
    assert int(HJ.lib().hj_solve_bytes()) == 432          # the header's scratch figure
