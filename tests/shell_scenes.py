"""The two-cloth scene of the shell bending and shell damping GPU tests, and the stiffness that puts dt at a share of the guard."""
import numpy as np

from tests import shell_bending as sb


def scale_k(g, set_with, dt, share=0.5):
    """k such that dt is `share` of mpm_shell_max_stable_dt (the limit scales with 1 / sqrt(k)); set_with(k) sets it"""
    set_with(1.0)
    lim = g.shell_max_stable_dt()
    assert np.isfinite(lim) and lim > 0
    k = float(np.float32((share * lim / dt) ** 2))
    set_with(k)
    assert abs(g.shell_max_stable_dt() * share / dt - 1.0) < 1e-3
    return k


def scene():
    """the tube and the book side by side: (cloths as added, rest_pos of all vertices, hinges in global ids, cloth of hinge)"""
    Xt, Tt, _ = sb.mesh("tube")
    Xb, Tb, rb = sb.mesh("book")
    st, sh = np.array([-0.15, 0.0, 0.0], np.float32), np.array([0.12, 0.0, 0.0], np.float32)
    cloths = [(Xt + st, Tt), (Xb + sh, Tb)]
    rest = np.concatenate([Xt + st, rb + sh])
    Ht, Hb = sb.hinges(Tt), sb.hinges(Tb) + len(Xt)
    return cloths, rest, np.concatenate([Ht, Hb]), np.concatenate([np.zeros(len(Ht), int), np.ones(len(Hb), int)])


def flying(seed=3):
    cloths, rest, H, ch = scene()
    x0 = rest.copy()
    v0 = np.array([4.0, 0.3, 0.0], np.float32) + 0.05 * np.random.default_rng(seed).normal(size=x0.shape).astype(np.float32)
    return cloths, rest, H, ch, x0, v0
