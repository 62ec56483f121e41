"""What the GPU tests of the cloth features share: one engine builder, one state upload, the views of the engine's arrays by
original id, the bit compare and the margin record.  drake_amd and tests.helpers are imported inside the functions, so
that collection needs neither the library nor a GPU."""
import contextlib
import os

import numpy as np


def ARR():
    from drake_amd import ARR
    return ARR


@contextlib.contextmanager
def environ(env):
    """the variables of `env` (None or a dict) set inside the block; what was there before is back after it"""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def engine(cloths, bits=6, material=None, mats=None, deterministic=True, fast_math=None, bodies=0, env=None):
    """A finalized engine.  cloths: [(X (n, 3) float32, T)] at rest or [(pos, vel, idx)] (vel None: at rest); material:
    fields of the engine's material; mats: per cloth a dict of ClothMaterial fields over the engine's, or None for the
    engine's material itself (any dict makes the engine multi-material); deterministic, fast_math: None leaves the
    setter uncalled; env: the environment around mpm_create alone.  g._tri: the faces (n_faces, 3) in engine numbering."""
    from drake_amd import ClothMaterial, GpuMpm
    mat = GpuMpm.default_material()
    for k, val in (material or {}).items():
        setattr(mat, k, val)
    with environ(env):
        g = GpuMpm(bits, mat)
    if deterministic is not None:
        g.set_deterministic(deterministic)
    if fast_math is not None:
        g.set_fast_math(fast_math)
    for c, cloth in enumerate(cloths):
        pos, vel, idx = cloth if len(cloth) == 3 else (cloth[0], None, cloth[1])
        m = None
        if mats is not None and mats[c] is not None:
            m = ClothMaterial.of(mat)
            for k, val in mats[c].items():
                setattr(m, k, val)
        g.add_qr_cloth(pos, np.zeros_like(pos) if vel is None else vel, idx, m)
    g.finalize()
    if bodies:
        g.reallocate_external_bodies(bodies)
    offs = np.cumsum([0] + [len(c[0]) for c in cloths[:-1]])
    g._tri = np.concatenate([np.asarray(c[-1]).reshape(-1, 3) + o for c, o in zip(cloths, offs)])
    return g


def upload(g, x, v=None, F=None):
    """vertex positions and velocities (n_verts, 3) in original order (v: also one 3-vector for all, None: zero); a face
    particle gets the float64 mean of its corners; C = 0; F: per face as upload_particle_state takes it, None: kept"""
    x = np.asarray(x, np.float32)
    v = np.zeros_like(x) if v is None else np.broadcast_to(np.asarray(v, np.float32), x.shape)
    mean = lambda a: a[g._tri].astype(np.float64).mean(axis=1).astype(np.float32)   # noqa: E731
    pos, vel = np.concatenate([mean(x), x]), np.concatenate([mean(v), v])
    pids = g.download(ARR().PIDS)
    g.upload_particle_state(pos[pids], vel[pids], np.zeros((len(pos), 9), np.float32), None, F)


def by_id(g, which, split=False):
    """a per-particle array of the engine in original order; split: (face part, vertex part)"""
    a, pids = g.download(which), g.download(ARR().PIDS)
    out = np.zeros_like(a)
    out[pids] = a
    return (out[:g.n_faces], out[g.n_faces:]) if split else out


def vertices(g, which):
    """a per-particle array of the engine, for the vertices in original order"""
    a, pids = g.download(which), g.download(ARR().PIDS)
    out = np.zeros((g.n_verts,) + a.shape[1:], a.dtype)
    out[pids[pids >= g.n_faces] - g.n_faces] = a[pids >= g.n_faces]
    return out


def state(g, bodies=False):
    """what a substep leaves behind, in the engine's order; bodies: also the reactions on the rigid bodies"""
    A = ARR()
    tau, f = g.external_body_force_to_host() if bodies else (None, None)
    s = dict(x=g.download(A.POSITIONS), v=g.download(A.VELOCITIES), C=g.download(A.AFFINE), pids=g.download(A.PIDS),
             F=g.download(A.DEFORMATION_GRADIENTS))
    if bodies:
        s.update(tau=tau, f=f)
    return s


def phases(g, dt, bc=-1):
    """one substep as the five phase calls"""
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(dt)
    g.particle_to_grid(dt)
    g.update_grid(bc)
    g.grid_to_particle(dt)


def bits(a):
    """the words of an array of 4-byte or 8-byte items (no cast)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b, what):
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))


def record(what, ratio, prefix=""):
    """one line of the margin table (tests/conftest.py): `ratio` of what the test allows"""
    from tests import helpers
    helpers.MARGINS.append((ratio, prefix + what + helpers.TAG, 1.0, ratio, ratio))
