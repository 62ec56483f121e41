"""Float64 restatement of the pin semantics of include/mpm_hip.h (mpm_set_pins, mpm_set_body_motions), and their
emulation on the host for the CPU oracle: after GridToParticle a pinned vertex is overwritten with the rigid target of its
body and the body collects the reaction.  Used by tests/test_pins.py and tests/test_pins_gpu.py."""
import numpy as np


def rodrigues(a):
    """rotation matrix exp([a]x) of a rotation vector a (float64)"""
    a = np.asarray(a, np.float64)
    th = float(np.linalg.norm(a))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    if th < 1e-8:
        s, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        s, c = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + s * K + c * (K @ K)


def skew(w):
    w = np.asarray(w, np.float64)
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def as_engine_sees(motion):
    """(p_WB, R_WB (3, 3), v, w) as float64 of the float32 values the engine is given"""
    p, R, v, w = motion
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return f(p).reshape(3), f(R).reshape(3, 3), f(v).reshape(3), f(w).reshape(3)


def pin_target(motion, p_BQ, t):
    """x, v_Q, C of an attachment point p_BQ (body frame) at clock t: p(t) = p_WB + t v, R(t) = Rodrigues(t w) R_WB,
    x = p(t) + R(t) p_BQ, v_Q = v + w x (x - p(t)), C = [w]x.  p_BQ: (3,) or (n, 3)."""
    p, R, v, w = as_engine_sees(motion)
    Rt = rodrigues(t * w) @ R
    pt = p + t * v
    r = np.asarray(p_BQ, np.float32).astype(np.float64) @ Rt.T
    x = pt + r
    vq = v + np.cross(w, r)
    return x, vq, skew(w)


class PinEmulator:
    """The pins of one engine on the host.  pins: list of (vertex, body, p_BQ); motions: {body: (p_WB, R_WB, v, w)}.
    apply(o, dt, nf, density) runs after the oracle's grid_to_particle: advances every clock by dt, overwrites the
    pinned vertices' pos / vel / C at o.index_mappings[nf + vertex] and returns {body: (tau, f)} of this substep
    (float64; torque about the body's p_WB)."""

    def __init__(self, pins, motions):
        self.pins = [(int(v), int(b), np.asarray(q, np.float32)) for v, b, q in pins]
        self.motions = dict(motions)
        self.t = {b: 0.0 for b in self.motions}

    def set_motions(self, motions):
        for b, m in motions.items():
            self.motions[b] = m
            self.t[b] = 0.0

    def apply(self, o, dt, nf, density):
        dt = float(np.float32(dt))
        for b in self.t:
            self.t[b] += dt
        out = {}
        for vtx, b, q in self.pins:
            s = int(o.index_mappings[nf + vtx])
            x, vq, Cm = pin_target(self.motions[b], q, self.t[b])
            m = float(o.vol[s]) * float(density)
            l = m * (np.asarray(o.vel[s], np.float64) - vq)
            p0 = as_engine_sees(self.motions[b])[0]
            tau = np.cross(x - p0, l)
            acc = out.setdefault(b, [np.zeros(3), np.zeros(3)])
            acc[0] += tau
            acc[1] += l
            o.pos[s] = x
            o.vel[s] = vq
            o.C[s] = Cm.reshape(9)
        return {b: (a[0], a[1]) for b, a in out.items()}


def face_recentring(vel, vol, indices, nf, density):
    """Momentum CalcFemStateAndForce adds by putting every face particle's velocity at the mean of its corners'
    (ids in Finalize order: vel / vol indexed by particle id, indices = corner ids)."""
    corners = np.asarray(indices).reshape(-1, 3)
    vbar = np.asarray(vel, np.float64)[corners].mean(axis=1)
    m = np.asarray(vol[:nf], np.float64) * float(density)
    return (m[:, None] * (vbar - np.asarray(vel[:nf], np.float64))).sum(axis=0)
