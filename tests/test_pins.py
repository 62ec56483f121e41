"""Fixed constraints (pins) without a GPU: the C ABI declares and exports the pin calls, the ctypes layouts match the
header, the float64 restatement of the rigid target (tests/pin_reference.py) holds for simple motions, and on the CPU
oracle with pins emulated on the host the grid momentum obeys the impulse the pins report."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.pin_reference import PinEmulator, face_recentring, pin_target, rodrigues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpm_set_pins", "mpm_set_body_motions", "mpm_pins_inside_collider", "mpm_get_pins")


def _header():
    return open(os.path.join(ROOT, "include", "mpm_hip.h")).read()


def test_pin_calls_are_declared_bound_and_exported():
    from drake_amd import capi
    text = _header()
    for name in NEW:
        assert re.search(r"MPM_API\s+int\s+" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS, name
    lib = capi.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    for m in ("set_pins", "set_body_motions", "pins_inside_collider", "get_pins"):
        assert hasattr(capi.GpuMpm, m), m


def _struct_layout(name):
    """(size, {field: offset}) of a header struct, from a host compile of the header"""
    import shutil
    import subprocess
    import tempfile
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    fields = {"mpm_pin_t": ("vertex", "body", "p_BQ"), "mpm_body_motion_t": ("body", "p_WB", "R_WB", "v", "w")}[name]
    src = "#include <cstddef>\n#include <cstdio>\n#include \"mpm_hip.h\"\nint main() {\n"
    src += f'  std::printf("%zu\\n", sizeof({name}));\n'
    for f in fields:
        src += f'  std::printf("{f} %zu\\n", offsetof({name}, {f}));\n'
    src += "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "l.cc"), os.path.join(d, "l")
        open(c, "w").write(src)
        subprocess.check_call([cc, "-std=c++17", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    return int(out[0]), {ln.split()[0]: int(ln.split()[1]) for ln in out[1:] if ln.strip()}


@pytest.mark.parametrize("name,cls", [("mpm_pin_t", "Pin"), ("mpm_body_motion_t", "BodyMotion")])
def test_ctypes_layouts_match_the_header(name, cls):
    from drake_amd import capi
    S = getattr(capi, cls)
    size, offs = _struct_layout(name)
    assert C.sizeof(S) == size
    for f, off in offs.items():
        assert getattr(S, f).offset == off, f


def test_rigid_target_identity_translation_and_quarter_turn():
    q = np.array([0.1, -0.2, 0.05])
    # identity: the attachment point sits where the body frame puts it, at rest
    x, v, Cm = pin_target(((0.3, 0.4, 0.5), np.eye(3), (0, 0, 0), (0, 0, 0)), q, 0.25)
    f64 = lambda a: np.float32(a).astype(np.float64)
    assert np.allclose(x, f64(q) + f64([0.3, 0.4, 0.5]), atol=0, rtol=1e-15)
    assert np.all(v == 0) and np.all(Cm == 0)
    # pure translation: x = p + t v, v_Q = v
    vel = (0.5, -0.25, 0.125)
    x, v, Cm = pin_target(((0.3, 0.4, 0.5), np.eye(3), vel, (0, 0, 0)), q, 2.0)
    assert np.allclose(x, f64([0.3, 0.4, 0.5]) + 2.0 * f64(vel) + f64(q), rtol=1e-15, atol=1e-16)
    assert np.allclose(v, vel) and np.all(Cm == 0)
    # 90 degrees about z after t = 1 at w = (0, 0, pi/2): x_B -> y_B, velocity w x r, C = [w]x (skew)
    w = (0.0, 0.0, np.pi / 2)
    x, v, Cm = pin_target(((0, 0, 0), np.eye(3), (0, 0, 0), w), (1.0, 0.0, 0.0), 1.0)
    assert np.allclose(x, [0.0, 1.0, 0.0], atol=1e-7)
    assert np.allclose(v, np.cross(np.float32(w), x), atol=1e-7)
    assert np.allclose(Cm, -Cm.T) and np.allclose(Cm @ x, v, atol=1e-7)
    # a starting rotation composes on the right: R(t) = Rodrigues(t w) R_WB
    R0 = rodrigues([0.0, 0.0, np.pi / 2]).astype(np.float32)
    x, _, _ = pin_target(((0, 0, 0), R0, (0, 0, 0), (np.pi / 2, 0, 0)), (1.0, 0.0, 0.0), 1.0)
    assert np.allclose(x, [0.0, 0.0, 1.0], atol=1e-6)


def _pinned_oracle(real, bits=6):
    from drake_amd import scenes
    from oracle import oracle as orc
    sheets = scenes.cloth_stack(2, 16, bits, z0=0.5, side=0.3, seed=7, vel_amp=0.2)
    o = orc.OracleMpm(bits, real=real)
    for pos, vel, idx in sheets:
        o.add_qr_cloth(pos, vel, idx)
    o.finalize()
    nf, nv = o.n_faces, o.n_verts
    verts = np.arange(0, nv, 20)   # 5 % of the vertices
    x0 = o.pos[nf + verts].astype(np.float64)
    p_WB = np.array([0.5, 0.5, 0.5])
    R_WB = rodrigues([0.1, 0.2, 0.3])
    pins = [(v, 0, R_WB.T @ (x0[k] - p_WB)) for k, v in enumerate(verts)]
    em = PinEmulator(pins, {0: (p_WB, R_WB, (0.05, -0.02, 0.01), (0.3, -0.2, 0.5))})
    return o, em


# Tolerances of the momentum identity, relative to M |g| dt, each a fixed multiple of the residual measured when this
# test was written (6 substeps of the scene below): float64 build 2.4e-14 (allowed 1e-12, ~40x), float32 build 7.6e-8
# (allowed 1e-6, ~13x).  Without the pins' impulse the residual is ~0.2, without the face re-centring term ~0.07.
MOMENTUM_RTOL = {np.float64: 1e-12, np.float32: 1e-6}


@pytest.mark.parametrize("real", [np.float64, np.float32])
def test_pins_momentum_identity_on_the_oracle(real):
    """P = sum of the grid momentum after ParticleToGrid.  Over a substep k with pins, and mpm_bc = -1 far from the
    walls, P_{k+1} - P_k = M g dt - l_k + d_{k+1}: l_k the summed force impulse the pins report for substep k, d_{k+1}
    the momentum CalcFemStateAndForce adds when it puts the face particles at the mean velocity of their corners (the
    pins change the corners' velocities after GridToParticle has set the faces')."""
    o, em = _pinned_oracle(real)
    nf, dens, dt = o.n_faces, float(o.p.density), 1e-3
    g = np.zeros(3)
    g[o.p.gravity_axis] = o.p.gravity
    P_prev = l_prev = None
    checked = 0
    for k in range(6):
        o.rebuild_mapping(False)
        st = o.state_in_original_order()
        d = face_recentring(st["vel"], st["vol"], o.indices, nf, dens)
        o.calc_fem_state_and_force(dt)
        o.particle_to_grid(dt)
        P = o.g_mv.astype(np.float64).sum(axis=0)
        M = float(o.g_m.astype(np.float64).sum())
        scale = M * abs(float(o.p.gravity)) * dt
        if P_prev is not None:
            r = P - P_prev - (M * g * dt - l_prev + d)
            assert np.abs(r).max() <= MOMENTUM_RTOL[real] * scale, (k, r, scale)
            assert np.abs(l_prev).max() > 0.05 * scale   # the pins do carry an impulse
            checked += 1
        o.update_grid(-1)
        o.grid_to_particle(dt)
        out = em.apply(o, dt, nf, dens)
        P_prev, l_prev = P, out[0][1]
    assert checked == 5
