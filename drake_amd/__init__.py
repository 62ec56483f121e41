"""drake_amd: MI355X-native cloth-MPM substep engine behind g1n0st/drake's
GpuMpmState / GpuMpmSolver interface.

The product is the C-ABI library built from drake_amd/csrc (see
include/mpm_hip.h).  This package only holds the build recipe, a ctypes binding
used by the tests and bench.py, and synthetic scene generators.  There is no
CPU fallback: every compute call goes to the HIP library or raises.
"""
from .capi import (MpmError, GpuMpm, load_library, library_path, Material, Collider, SdfCollider, GridCollider, BC_TABLE,  # noqa: F401
                   grid_collider_preset, ARR, RT, PHASES, Pin, BodyMotion, ClothMaterial, GridBody, BC_BODIES, GB_NO_MESH, ForceField,
                   force_field_acceleration, FF_ACCEL, FF_DRAG, FF_NORMAL_DRAG, FF_QUADRATIC, FF_REGION, bending_matrix,
                   cloth_energy_density, MEASURE_DTYPE, damping_face_records, LINK_DTYPE, LINK_TENSION_ONLY, links,
                   link_force, PRESSURE_DTYPE, PRESSURE_STATE_DTYPE, PRESSURE_OFF, PRESSURE_CONSTANT, PRESSURE_GAS,
                   mesh_is_closed, pressure_vertex_force, SHELL_DTYPE, SHELL_REST_SHAPE, SHELL_REST_FLAT, mesh_hinges,
                   shell_hinge, Anchor, ANCHOR_DTYPE, ANCHOR_TENSION_ONLY, anchor_point, WEAVE_DTYPE, weave,
                   weave_coefficients, weave_face_records, weave_face_axes, TEAR_DTYPE, tear_face, tear_limit_squared,
                   link_breaks, link_break_squared, rest_shape_check, CREASE_DTYPE, crease, crease_chord, crease_hinge,
                   TEAR_CUTS_HINGES, TEAR_VENTS_GAS, mesh_hinge_faces, SHELL_DAMPING_DTYPE, shell_hinge_damped)
from . import scenes  # noqa: F401
