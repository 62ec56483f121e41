"""External force fields on the CPU: the library exports the entry points, mpm_force_field_acceleration (the inline
function k_p2g calls, compiled for the host) agrees with the float64 restatement of tests/force_fields.py per particle
within the rounding bound, the extended node bound is not too tight for honest float32 arithmetic, and every invalid
table is refused."""
import os

import numpy as np
import pytest

from tests import force_fields as ff
from tests import harness as hs
from tests import transfer_layouts as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("dense", "kinds", "materials", "magnitudes")


def _c(fields):
    from drake_amd import ForceField
    return [ForceField(kind=f["kind"], gamma=float(f["gamma"]), u0=f["u0"], G=f["G"], x0=f["x0"],
                       region=(f["lo"], f["hi"]) if f["flags"] & ff.FF_REGION else None, flags=f["flags"]) for f in fields]


def test_library_exports_the_force_field_entry_points():
    import ctypes
    from drake_amd import capi
    lib = capi.load_library()
    for name in ("mpm_set_force_fields", "mpm_get_force_fields", "mpm_force_field_acceleration"):
        assert name in capi.SYMBOLS
        assert hasattr(lib, name), name
    # the binding's structure is the header's: 24 packed 4-byte members
    assert ctypes.sizeof(capi.ForceField) == 96
    text = open(os.path.join(ROOT, "include", "mpm_hip.h")).read()
    for name in ("MPM_FF_ACCEL 0", "MPM_FF_DRAG 1", "MPM_FF_NORMAL_DRAG 2", "MPM_FF_QUADRATIC 1u", "MPM_FF_REGION 2u",
                 "MPM_MAX_FORCE_FIELDS 8"):
        assert "#define " + name in text, name
    assert (capi.FF_ACCEL, capi.FF_DRAG, capi.FF_NORMAL_DRAG, capi.FF_QUADRATIC, capi.FF_REGION) == (0, 1, 2, 1, 2)


def _particles(seed, n=10_000):
    rng = np.random.default_rng(seed)
    x = tl.f32(rng.uniform(0.3, 0.7, (n, 3)))
    v = tl.f32(rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 1, (n, 1)))
    d = rng.normal(size=(n, 3))
    d = tl.f32(d * rng.uniform(0.5, 1.5, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    d[7] = 0.0   # a face with no director: normal drag contributes nothing
    return x, v, d


@pytest.mark.parametrize("kind", ("faces", "vertices"))
@pytest.mark.parametrize("name", ff.TABLES)
def test_host_evaluation_against_float64(name, kind):
    """every component of every particle within K (R + 2) u x its sum of absolute terms; no particle left out"""
    from drake_amd import force_field_acceleration
    x, v, d = _particles(100 + ff.TABLES.index(name))
    fields = ff.table(name)
    faces = kind == "faces"
    got = force_field_acceleration(_c(fields), x, v, d if faces else None)
    a64, T = ff.accel64(fields, x, v, d if faces else None, faces)
    assert np.isfinite(got).all()
    w = tl.margin(np.abs(got.astype(np.float64) - a64), ff.accel_bound(T))
    hs.record(f"force fields: host evaluation {name} [{kind}]", w)
    assert w <= 1.0, w
    # where no field acts the result is exactly zero, and the table does act on a good part of the particles
    assert (got[(T == 0).all(axis=1)] == 0).all()
    if not (name.startswith("normal") and not faces):
        assert (T > 0).any(axis=1).mean() > 0.1
    else:
        assert (got == 0).all()
    if faces and name.startswith("normal"):
        assert (got[7] == 0).all() and (a64[7] == 0).all()


def test_host_evaluation_table_order_and_region_edges():
    """a particle exactly on a region's face is inside (closed box); an empty table gives zero"""
    from drake_amd import force_field_acceleration
    f = ff.field(ff.FF_ACCEL, u0=(1.0, 2.0, 3.0), region=((0.25, 0.25, 0.25), (0.5, 0.5, 0.5)))
    x = tl.f32([[0.25, 0.5, 0.3], [np.nextafter(np.float32(0.25), np.float32(0)), 0.5, 0.3],
                [0.3, np.nextafter(np.float32(0.5), np.float32(1)), 0.3]])
    got = force_field_acceleration(_c([f]), x, np.zeros_like(x))
    assert np.array_equal(got, tl.f32([[1, 2, 3], [0, 0, 0], [0, 0, 0]]))
    assert np.array_equal(force_field_acceleration([], x, x), np.zeros_like(x))


@pytest.mark.parametrize("table", ff.TABLES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_float32_restatement_within_the_extended_node_bound(name, table):
    """the float32 numpy restatement of the fields, pushed through p2g64's sums, stays within the extended node bound
    (the bound is not too tight for honest float arithmetic), and so does the library's host evaluation"""
    from drake_amd import force_field_acceleration
    lay = tl.layout(name)
    fields = ff.table(table, *ff.bbox(lay["pos"]))
    d = ff.layout_directors(lay)
    face = np.arange(lay["nf"] + lay["nv"]) < lay["nf"]
    args = (lay["pos"], lay["vel"], lay["C"], lay["mass"], lay["taus"], lay["forces"], d, face, lay["bits"], lay["gravity_axis"])
    r, a64, T = ff.p2g64_fields(fields, *args)
    _, bmv = ff.p2g_bounds(r, None, L=r["N"])
    a32 = ff.accel32(fields, lay["pos"], lay["vel"], d, face)
    nf = lay["nf"]
    lib = np.concatenate([force_field_acceleration(_c(fields), lay["pos"][:nf], lay["vel"][:nf], d[:nf]),
                          force_field_acceleration(_c(fields), lay["pos"][nf:], lay["vel"][nf:], None)])
    for what, a in (("numpy float32", a32), ("host evaluation", lib)):
        # m (a dt) as the kernel forms it, in float32
        imp = tl.f32(lay["mass"])[:, None] * (tl.f32(a) * np.float32(tl.DT32))
        r2, _, _ = ff.p2g64_fields(fields, *args, accel=imp.astype(np.float64) / (lay["mass"].astype(np.float64)[:, None] * tl.DT32))
        w = tl.margin(np.abs(r2["mv"] - r["mv"]), bmv)
        hs.record(f"force fields: {what} within the node bound: {name} {table}", w)
        assert w <= 1.0, (what, w)
    # the table reaches the layout: some particle inside and (regions) some outside every regioned field
    assert (T > 0).any()
    if table == "regions":
        on = [ff._member(f, tl.f32(lay["pos"]), face) for f in fields]
        assert on[0].any() and not on[0].all() and on[1].any() and not on[1].all() and not on[2].any()
        assert on[3].any() and not on[3][face].all()


def test_extended_bound_sees_a_missing_field():
    """the bound is tight enough to see a field that is left out"""
    lay = tl.layout("dense")
    fields = ff.table("drag_wind", *ff.bbox(lay["pos"]))
    d = ff.layout_directors(lay)
    face = np.arange(lay["nf"] + lay["nv"]) < lay["nf"]
    args = (lay["pos"], lay["vel"], lay["C"], lay["mass"], lay["taus"], lay["forces"], d, face, lay["bits"], lay["gravity_axis"])
    r, a64, _ = ff.p2g64_fields(fields, *args)
    _, bmv = ff.p2g_bounds(r, tl.fixed_quanta(lay["mass"]))
    r0, _, _ = ff.p2g64_fields(fields, *args, accel=np.zeros_like(a64))
    assert tl.margin(np.abs(r0["mv"] - r["mv"]), bmv) > 100


def _bad_tables():
    ok = dict(kind=ff.FF_DRAG, gamma=1.0)
    from drake_amd import ForceField
    out = {}
    out["unknown kind"] = [ForceField(kind=3)]
    out["negative kind"] = [ForceField(kind=-1)]
    out["unknown flags"] = [ForceField(flags=4, **ok)]
    for what, kw in (("gamma nan", dict(kind=ff.FF_DRAG, gamma=float("nan"))), ("u0 inf", dict(u0=(0, float("inf"), 0), **ok)),
                     ("G nan", dict(G=[0, 0, 0, 0, float("nan"), 0, 0, 0, 0], **ok)), ("x0 inf", dict(x0=(float("-inf"), 0, 0), **ok)),
                     ("lo nan", dict(region=((float("nan"), 0, 0), (1, 1, 1)), **ok)),
                     ("hi inf", dict(region=((0, 0, 0), (1, float("inf"), 1)), **ok))):
        out[what] = [ForceField(**kw)]
    out["gamma < 0"] = [ForceField(kind=ff.FF_DRAG, gamma=-1e-3)]
    out["lo > hi"] = [ForceField(region=((0, 0.6, 0), (1, 0.5, 1)), **ok)]
    out["n = 9"] = [ForceField(**ok) for _ in range(9)]
    out["second field bad"] = [ForceField(**ok), ForceField(kind=7)]
    return out


@pytest.mark.parametrize("what", ("unknown kind", "negative kind", "unknown flags", "gamma nan", "u0 inf", "G nan", "x0 inf",
                                  "lo nan", "hi inf", "gamma < 0", "lo > hi", "n = 9", "second field bad"))
def test_invalid_tables_are_refused(what):
    from drake_amd import MpmError, force_field_acceleration
    x = np.full((2, 3), 0.5, np.float32)
    with pytest.raises(MpmError) as e:
        force_field_acceleration(_bad_tables()[what], x, x)
    assert e.value.code == -1, e.value   # MPM_ERR_INVALID
    assert str(e.value)


def test_valid_edge_tables_are_accepted():
    from drake_amd import ForceField, force_field_acceleration
    x = np.full((2, 3), 0.5, np.float32)
    force_field_acceleration([ForceField(kind=ff.FF_DRAG, gamma=0.0, region=((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)))] * 8, x, x)
