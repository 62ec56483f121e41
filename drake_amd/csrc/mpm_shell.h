// Shell bending about a curved rest shape (mpm_set_shell_bending, include/mpm_hip.h): the discrete-shells hinge model
// (Grinspun et al. 2003, "Discrete shells") in the variable psi = 2 sin(theta / 2) (hinge energies in a function of
// theta and the gradient of theta: Tamstorf and Grinspun 2013, "Discrete bending forces and their Jacobians").  Hinges
// are those of mpm_set_bending: every edge shared by exactly two faces of one cloth; boundary edges and edges with more
// than two faces form none.  A hinge is (x0, x1 | x2, x3): x0 -> x1 is the edge as face A, the face with the lower id,
// runs it, x2 is opposite the edge in face A, x3 in face B; the hinges of all cloths with k > 0 are numbered in ascending
// (cloth, min(v0, v1), max(v0, v1)).
// All quantities are differences against x0 (translation invariant to the bit):
//   e = x1 - x0,  a = x2 - x0,  b = x3 - x0,   nA = e x a,  nB = b x e                 (parallel on a flat hinge)
//   nAh = nA / |nA|,  nBh = nB / |nB|,  sigma = +1 where e . (nA x nB) >= 0, else -1
//   psi  = sigma |nAh - nBh|   = 2 sin(theta / 2),  theta = atan2(e^ . (nA x nB), nA . nB) the signed dihedral angle
//   dpsi = 1/2 |nAh + nBh|     = cos(theta / 2) = d psi / d theta
//   E_h  = 1/2 k cbar (psi - psibar)^2,   cbar = 3 |ebar|^2 / (Abar_A + Abar_B)   (rest edge length and rest areas)
//   f_j  = -k cbar (psi - psibar) dpsi G_j,   G_j = grad_{x_j} theta:
//     G2 = -|e| nA / |nA|^2,  G3 = -|e| nB / |nB|^2,  with wA = a . e / |e|^2,  wB = b . e / |e|^2
//     G1 = -(wA G2 + wB G3),  G0 = -((1 - wA) G2 + (1 - wB) G3)                       (G0 + G1 + G2 + G3 = 0)
// No trigonometric function: square roots and divisions only, correctly rounded whatever mpm_set_fast_math says,
// every operation written out, contraction off (shell_hinge below: what k_hinge calls and what the host entry
// mpm_shell_hinge runs).  Five square roots and five divisions per hinge.
//
// Why 2 sin(theta / 2): with psibar = 0 the energy of a hinge whose two triangles move rigidly is exactly the quadratic
// model's 1/2 k c |K x|^2 (mpm_bending.h), so the same k means the same thing in both calls and this model is the
// quadratic one's rotation-invariant continuation to curved rest shapes; and it is bounded: no infinite force.
// ITS WEAKNESS: dpsi -> 0 as |theta| -> pi, so a hinge folded flat onto itself feels no restoring force, and psi jumps
// from 2 to -2 there: the energy is discontinuous for psibar != 0 while the force is continuous.
//
// The rest shape is an exact equilibrium: psibar is not computed on the host -- mpm_set_shell_bending runs the hinge
// function on the device once on the rest positions (k_hinge_rest) and keeps the psi it wrote, so on the rest positions
// psi - psibar is an exact zero and every record and every vertex force is +-0.  cbar is formed in double on the host
// and the product k cbar rounded to float once.  A hinge acts only while |e|^2, |nA|^2 and |nB|^2 are all >= 1e-30;
// otherwise its four records are exact zeros, its psi is 0 and it counts as inactive: never a NaN or an infinity.
//
// Device, two passes behind k_pressure in launch_fem_vertices, no atomics but the error flag, both starting with
// gated_out(p).  k_hinge, one lane per hinge in hinge order: four ids from the host-built table, four slots through
// DP::imap, four positions -- three round trips of independent loads --, then four corner records as float4 into four
// planes rec[j][h] (coalesced 16-byte stores); the .w of plane 0 carries psi, that of plane 1 the hinge's energy term
// 1/2 kc (psi - psibar)^2, that of plane 2 is 1 for a hinge that acts and 0 otherwise.  k_hinge_gather, one lane per
// row of a vertex row table (mpm_row_table.h, RowTable<uint32_t>: one row per vertex of the cloths with k > 0, a record
// is hinge << 2 | corner in ascending hinge id, padding 0xFFFFFFFF adds nothing and reads nothing), reads 8 records at a
// time and adds the records in stored order to DP::f.  Two passes because one evaluation per hinge then serves its four
// vertices (a one-pass gather would run shell_hinge four times per hinge, once per corner) and psi and the energy come
// for free; the price is 64 bytes written and read per hinge.  Table and order are those of the original ids: records,
// psi and forces are the same bits whatever the particle order.
//
// THE dt GUARD (mpm_shell_max_stable_dt): dt <= 2 / sqrt(max_i (1 / m_i) sum_{h contains i} kc dpsibar^2 |Gbar_hi|
// sum_j |Gbar_hj|), Gershgorin on the Gauss-Newton part of the stiffness, kc dpsi^2 G G^T, taken AT THE REST SHAPE
// (max_row_rate).  It does not cover the geometric stiffness (psi - psibar) d(dpsi G) / dx of a deformed hinge, nor a
// deformed hinge's larger |G| (|G2| = |e| / |nA| grows as a triangle collapses): a guard, not a guarantee.  At the rest
// shape it is between 0.58 and 0.81 of the true limit of this force alone; it says nothing about this force together
// with another ("What the dt guards bound").  It is NOT recomputed when hinges are cut (below) and stays a bound: every term
// of a row's Gershgorin sum is non-negative, so a row that loses hinges only loses terms.
//
// CUT HINGES (mpm_set_tear_coupling with MPM_TEAR_CUTS_HINGES, mpm_shell_cut_hinges): on a cloth that tears (mpm_tear.h) a
// hinge one of whose two faces is torn carries no moment.  "Cut" is not stored: it is torn[face A] | torn[face B],
// evaluated by k_hinge and k_crease in every substep from the tear flags (one byte per original face id) through a
// host-built table of the hinges' two GLOBAL face ids (HingeArgs::faces), so scissors and restore (mpm_set_torn_faces)
// need no code of their own and a re-sort moves nothing.  A cut hinge is an unusable one: its four records are +0, its
// psi 0, its energy term 0, plane 2's .w 0 (it counts as inactive); plane 3's .w, spare until now, is 1 for it and 0
// otherwise, which is where mpm_shell_cut_hinges reads the cut state.  k_crease: a cut hinge does not yield and keeps its
// psibar, so a hinge restored by mpm_set_torn_faces acts again with the psibar it had.  The pointer to the flags is put
// into a copy of the arguments per launch and is null unless the mode is set and the tear tables exist: a null pointer is
// the arithmetic, the loads and the stores of an engine without the mode.  ORDER: k_tear runs last of the face kernels,
// k_crease and k_hinge among the vertex kernels behind them, so a face that fails in a substep cuts its hinges in that
// same substep.  k_hinge_gather is unchanged.
//
// Roundings of one component of one record, for the bound of tests/shell_bending.py, first order, in units of 2^-24 of
//   T = |kc| |G_hj| (kappa_A + kappa_B) (1 + |psi| + |psibar|),   kappa_A = |e| |a| / |nA|,  kappa_B = |e| |b| / |nB|
// (the conditioning of the two normals; kappa >= 1, so kappa_A + kappa_B >= 2 and a plain relative rounding of a
// quantity bounded by |kc| |G_hj| (|psi| + |psibar|) costs at most 1/2 unit):
//   a normal: a component p - q of e x a carries the roundings of e and a (1 + 1), of each product (1) and of the
//     subtraction (1) on |p| + |q|, and the vector of those |p| + |q| is at most sqrt(2) |e| |a| long: 4 sqrt(2) < 6
//     kappa in the direction and the length of a normal
//   psi: the directions of nAh and nBh, 6 kappa each                                                                 6
//        their lengths (|n|^2: 3 on the square, 1.5 on the root; the root 1; the reciprocal 1; the product 1 = 4.5
//        each, which enter |nAh - nBh| at most as they are), the subtraction (1), |d|^2 and its root (2.5):
//        12.5 in all, at most 6.25 (kappa_A + kappa_B)                                                              6.25
//        psi - psibar: one rounding of at most |psi| + |psibar|                                                      0.5
//   dpsi, an absolute error that multiplies |kc| |psi - psibar| |G|: directions 6 kappa each, halved                   3
//        lengths 4.5 each, halved; the sum (1), |s|^2 and its root (2.5), the half (0): 8 in all, at most              4
//   m = -(kc (psi - psibar)) dpsi: two products                                                                       1
//   G2 = -(|e| / |nA|^2) nA: |e| (e: 1, |e|^2: 1.5, the root: 1 = 3.5), |nA|^2 (twice the normal's 6 kappa, and 3),
//        the division (1), nA's component (6 kappa), the product (1): 18 kappa + 9.5, at most 18 (kappa_A + kappa_B)
//        - 18 + 9.5 < 18 (kappa_A + kappa_B); likewise G3                                                             18
//   the record m G_j: one product                                                                                   0.5
//   corners 0 and 1: wA = (a . e) / |e|^2 (the dot product 4 on |a| |e|, |e|^2 3, the reciprocal 1, the product 1),
//        1 - wA (1), two products and their sum (2): counted on |wA| |G2| + |wB| |G3|, which is |G_hj| where the two
//        terms do not cancel                                                                                          6
//   second-order terms                                                                                               0.75
// R_shell = 46.  A row with n records adds them in stored order, one rounding of a partial sum per record, each partial
// sum at most the row's sum of T: R_i = 46 + n_i.  psi alone: at most 13 (kappa_A + kappa_B) (1 + |psi|) 2^-24.
//
// CREASES (mpm_set_creases, mpm_set_crease_state, mpm_crease_state, mpm_crease_measure, mpm_crease_hinge): plastic hinges.
// psibar, the number par[h].y that k_hinge reads, evolves under a yield rule on the generalised moment conjugate to theta,
// kc (psi - psibar) dpsi, per hinge with its cloth's (y, eta, P) (y = float(2 sin(yield_angle / 2)), eta the hardening
// ratio in [0, 1), P = float(2 sin(max_angle / 2)), formed in double on the host and rounded once).  crease_return below:
//   d = psi - psibar,  ad = |d|,  t = ad dpsi,  the hinge YIELDS where it acts, y > 0 and t > y (never on a NaN); then
//   dy = y / dpsi,  dn = dy + eta (ad - dy),  psibar' = clamp(psi - copysign(dn, d), -P, P);  otherwise psibar' = psibar.
// A return mapping: it runs BEFORE the force (k_crease immediately in front of k_hinge), so from the substep in which a
// hinge yields its moment is at most kc (y + eta (t - y)), up to rounding; psibar moves towards psi and never past it
// (dy < ad wherever t > y, and eta < 1).  On the moment and not on psi - psibar alone because dpsi -> 0 as |theta| -> pi:
// a hinge folded flat onto itself, where psi jumps between +2 and -2, carries no moment and does not yield, so a sheet
// folded in half does not flip its crease when theta wobbles across pi.  eta is the post-yield tangent over the elastic
// one: 0 is perfectly plastic.
// k_crease, one lane per hinge, 256 per block, gated_out(p) first, launched only while the crease tables exist: a lane
// whose y is 0 returns at once; any other reads the four ids (and its psibar), the four slots through DP::imap and the
// four positions -- three round trips of independent loads, the id and slot checks of hinge_on_state --, runs shell_angle
// (shell_hinge's operations up to psi and dpsi, restated: the same bits) and crease_return, and stores par[h].y where the
// hinge yields: a plain 4-byte store, one writer per hinge, no atomics but the error flag, no LDS.  Decisions are taken
// hinge by hinge on the positions of the substep's start (Jacobi), so the result does not depend on the particle order or
// on deterministic mode; a substep that skips itself changes nothing (with eta > 0 the update is not idempotent).
// k_crease_eval (mpm_crease_measure): the same function without the gate and without the store.
// The cost of k_crease on an MI355X: 14.8 us per substep on cloth_1m with shell bending on every sheet (990,720 hinges, a
// yield angle set, no hinge yielding); k_hinge behind it finds the ids and positions in the L2 and runs 4 us shorter
// (profiles/creases.txt).  A substep in which many hinges yield has not been measured.
// NOT MODELLED: no rate dependence (no creep, no viscoplasticity), no softening (a crease never weakens the hinge), no
// coupling between neighbouring hinges (each yields on its own moment), and the psi discontinuity at |theta| = pi of the
// elastic model above stays: a crease with psibar != 0 sees the same jump of the energy there.
// Roundings, for the bounds of tests/creases.py, first order, in units of 2^-24 of
//   W = (kappa_A + kappa_B) (1 + |psi| + |psibar|)        (kappa_A + kappa_B >= 2: one rounding of a quantity bounded by
//                                                          |psi| + |psibar| costs at most 1/2 unit)
//   t: psi (above), times dpsi <= 1                                                                                  13
//      d = psi - psibar: one rounding                                                                                0.5
//      dpsi's absolute error (the "dpsi" lines above: 3 + 4), times ad <= |psi| + |psibar|                             7
//      the product ad dpsi                                                                                           0.5
//      second-order terms                                                                                              1
// R_crease_t = 22: |t - t64| <= 22 W 2^-24; a hinge with |t64 - y| within that is UNDECIDED.
//   psibar' of a hinge that yields, in units of W / dpsi (1 / dpsi >= 1 multiplies what enters through dy = y / dpsi):
//      psi, which enters psi - copysign(dn, d) as (1 - eta) psi                                                       13
//      d: one rounding, times eta                                                                                    0.5
//      dy: dpsi's relative error 7 (kappa_A + kappa_B) / dpsi on dy < ad, times (1 - eta)                              7
//          the division's rounding                                                                                   0.5
//      the hardening line dy + eta (ad - dy): three roundings of at most ad                                          1.5
//      the final subtraction, |psibar'| <= max(|psi|, |psibar|)                                                      0.5
//      second-order terms                                                                                              1
// R_crease = 24: |psibar' - psibar'64| <= 24 W / dpsi 2^-24 (the clamp is monotone and 1-Lipschitz: it adds nothing).
//
// HINGE DAMPING (mpm_set_shell_damping, mpm_shell_damping_forces, mpm_shell_damping_state, mpm_shell_hinge_damped):
// stiffness-proportional damping of these hinges, per cloth, beta in seconds.  Not a feature of its own: state of shell
// bending, as creases are -- the tables go with the hinge table they belonged to.  Per hinge of a cloth with beta > 0, with
// the corner velocities as differences against corner 0 (Galilean invariant to the bit), w_j = v_j - v_0:
//   thetadot = sum_j G_j . v_j = G2 . (w2 - wA w1) + G3 . (w3 - wB w1) = -(gA nA . (w2 - wA w1) + gB nB . (w3 - wB w1))
//   psidot   = dpsi thetadot
//   m_d      = -(bkc psidot) dpsi,     bkc = float(beta k cbar), formed in double on the host and rounded once
//   f_j      = (m_el + m_d) G_j,       m_el = -(kc (psi - psibar)) dpsi as above
// which is -beta times the Gauss-Newton stiffness kc dpsi^2 G G^T applied to the velocities: the matrix the guard bounds,
// the stiffness half of a Rayleigh pair.  Linear in v, an exact zero for a common velocity, zero up to rounding for a
// rigid rotation, dissipative (-sum_j f_j . v_j = bkc psidot^2 >= 0), bounded where the elastic force is and gone where
// dpsi -> 0.  THE ORDER OF OPERATIONS (shell_hinge_core below, MODE != 0; contraction off, every division correctly
// rounded): the geometry exactly as shell_hinge forms it up to wA and wB; then per component k
//   w1 = v1 - v0, w2 = v2 - v0, w3 = v3 - v0;   p2 = w2 - wA * w1,  p3 = w3 - wB * w1;
//   sA = (nA[0] * p2[0] + nA[1] * p2[1]) + nA[2] * p2[2],  sB likewise with nB and p3;
//   thetadot = -(gA * sA + gB * sB);  psidot = dpsi * thetadot;  m_d = -(bkc * psidot) * dpsi;
//   m = bkc != 0 ? m_el + m_d : m_el   (a SELECTION: a hinge with bkc = 0 gives shell_hinge's bits, whatever its
//   velocities, a NaN included, and no signed zero is added);  the four records from m as shell_hinge forms them.
// One evaluation and one set of four records per hinge: k_hinge_gather is unchanged.  An unusable or cut hinge writes exact
// zeros as before, so a cut hinge is not damped.  The hinge's power term is the float (bkc * psidot) * psidot.
// k_hinge is a template on the mode: k_hinge<0> is the kernel without damping (the same loads, arithmetic and stores);
// k_hinge<1>, launched in its place while a cloth has beta > 0, also loads the four corner velocities from S.q[1] in the
// round trip of the four positions -- still three dependent round trips -- and bkc from HingeArgs::bkc beside the ids.
// HingeArgs::bkc is set in the per-launch copy of the arguments and is null while the damper is off.  k_hinge_eval<2>
// (mpm_shell_damping_forces, mpm_shell_damping_state) leaves m_el out and reuses the record planes, which every substep
// rewrites before it reads them: plane 0's .w is psidot, plane 1's the power term; a null bkc is bkc = 0 there.
// NOT MODELLED: no mass-proportional part; the damping moment does not enter the crease yield rule (k_crease is untouched
// and yields on the elastic moment alone); the geometric stiffness is not damped.
// THE dt GUARD with damping: symplectic Euler on x'' = -W x - G x' is stable iff W dt^2 + 2 G dt <= 4 (link_limit,
// mpm_links.h); W is the elastic guard's max row rate, G the same maximum with every row's sum times its cloth's beta (a
// row's hinges all belong to one cloth).  While no cloth has beta > 0 the limit is the elastic expression, to the bit.
// Like the elastic guard it holds at the rest shape, for this force alone, and is not a guarantee; the stiffness and the
// damping matrix do not commute once cloths differ in beta, and the root is a bound all the same ("What the dt
// guards bound", has the measured margins).
// Roundings of one component of one record of the damping part, for the bound of tests/shell_damping.py, first order, in
// units of 2^-24 of
//   D = |bkc| dpsi |G_hj| V (kappa_A + kappa_B),   V = |G2| (|w2| + (|a| / |e|) |w1|) + |G3| (|w3| + (|b| / |e|) |w1|)
// (the atoms are the differences e, a, b, w_j; V bounds |thetadot| and every partial sum on the way, |a| / |e| >= |wA|
// because wA's own error is relative to |a| |e| / |e|^2 and not to |wA|; V >= sum_j |G_j| |w_j|, with equality up to the
// cancellation inside G1.  dpsi <= 1 and kappa_A + kappa_B >= 2: a plain relative rounding of the result costs 1/2):
//   thetadot, per side, relative to |G2| (|w2| + (|a| / |e|) |w1|):
//        w1 (1), wA (the dot product 4, |e|^2 3, the reciprocal 1, the product 1 = 9), wA * w1 (1), w2 and the
//        subtraction (1 + 1, on the other part: the larger part counts)                                  12
//        nA's components 6 kappa_A, the dot product nA . p2 (3)                                 6 kappa + 3
//        gA = |e| / |nA|^2 (|e| 3.5, |nA|^2 12 kappa + 3, the division 1)                    12 kappa + 7.5
//        the product gA * sA                                                                              1
//        18 kappa + 23.5 <= 18 (kappa_A + kappa_B) - 18 + 23.5 <= 20.75 (kappa_A + kappa_B)                      20.75
//        the sum of the two sides (1 rounding of at most V)                                                        0.5
//   psidot = dpsi * thetadot: dpsi's absolute error (3 + 4 above) times |thetadot| <= V, the product (0.5)          7.5
//   m_d = -(bkc * psidot) * dpsi: the product (0.5), dpsi's absolute error again (7), the product (0.5)               8
//   m = m_el + m_d: one rounding of at most |m_el| + |m_d|, 0.5 here and 0.5 on T (above)                           0.5
//   G2 / G3 (18), the record m G_j (0.5), corners 0 and 1 (6), as for R_shell                                      24.5
//   second-order terms                                                                                             0.75
// R_shell_damp = 62.5: a damped hinge's record lies within ((R_shell + 0.5) T + 62.5 D) 2^-24 of the float64 one, the
// damping part alone (k_hinge_eval<2>) within 62 D 2^-24; a row adds its n_i.  psidot alone: at most 29 V (kappa_A +
// kappa_B) 2^-24.  Second order is NOT covered where dpsi itself is of the order of its error (|theta| within 1e-5 of pi).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mpm_row_table.h"

#ifdef __HIPCC__
#define MPM_SHELL_FN __host__ __device__ inline
#else
#define MPM_SHELL_FN inline
#endif

namespace mpm {

constexpr unsigned SHELL_REST_SHAPE = 0u, SHELL_REST_FLAT = 1u;   // mpm_cloth_shell_t::rest
constexpr int SHELL_SLICE = 64, SHELL_BATCH = 8;
constexpr uint32_t SHELL_PAD = 0xFFFFFFFFu;   // the gather table's padding record
constexpr float SHELL_GATE = 1e-30f;          // a hinge acts while |e|^2, |nA|^2, |nB|^2 >= this
constexpr float R_SHELL = 46.f;               // the counted roundings of one record (above)
constexpr float R_CREASE_T = 22.f, R_CREASE = 24.f;   // ... of a crease's t and of its psibar' (above)
constexpr float R_SHELL_DAMP = 62.5f, R_SHELL_PSIDOT = 29.f;   // ... of a record's damping part and of psidot (above)

struct ClothShell {   // mirrors mpm_cloth_shell_t (include/mpm_hip.h)
    float stiffness;
    uint32_t rest;
};
struct ClothCrease {   // mirrors mpm_cloth_crease_t
    float yield_angle, hardening, max_angle, reserved;
};
struct ClothShellDamping {   // mirrors mpm_cloth_shell_damping_t
    float beta, reserved;
};

// The four corner records rec[j] = f_j of one hinge and its psi; kc = float(k cbar).  false: the hinge does not act
// (the records and psi are exact zeros).  No branch on the data but the final selections.
// MODE 0: the elastic hinge, no velocity is read (v may be null).  MODE 1: the damped hinge (the header, HINGE DAMPING):
// v[4][3] the corner velocities, bkc = float(beta k cbar); *psidot_out = psidot, *power_out = (bkc psidot) psidot, zeros
// for a hinge that does not act.  MODE 2: the damping part alone (m_el left out).
template <int MODE>
MPM_SHELL_FN bool shell_hinge_core(const float x0[3], const float x1[3], const float x2[3], const float x3[3], const float (*v)[3],
                                   float kc, float psibar, float bkc, float rec[4][3], float* psi_out, float* psidot_out,
                                   float* power_out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float e0 = x1[0] - x0[0], e1 = x1[1] - x0[1], e2 = x1[2] - x0[2];
    const float a0 = x2[0] - x0[0], a1 = x2[1] - x0[1], a2 = x2[2] - x0[2];
    const float b0 = x3[0] - x0[0], b1 = x3[1] - x0[1], b2 = x3[2] - x0[2];
    // nA = e x a, nB = b x e
    const float A0 = e1 * a2 - e2 * a1, A1 = e2 * a0 - e0 * a2, A2 = e0 * a1 - e1 * a0;
    const float B0 = b1 * e2 - b2 * e1, B1 = b2 * e0 - b0 * e2, B2 = b0 * e1 - b1 * e0;
    const float ee = (e0 * e0 + e1 * e1) + e2 * e2;
    const float AA = (A0 * A0 + A1 * A1) + A2 * A2;
    const float BB = (B0 * B0 + B1 * B1) + B2 * B2;
    const bool on = (ee >= SHELL_GATE) & (AA >= SHELL_GATE) & (BB >= SHELL_GATE);
    const float le = sqrtf(ee), lA = sqrtf(AA), lB = sqrtf(BB);
    const float rA = 1.f / lA, rB = 1.f / lB;
    const float hA0 = A0 * rA, hA1 = A1 * rA, hA2 = A2 * rA;
    const float hB0 = B0 * rB, hB1 = B1 * rB, hB2 = B2 * rB;
    const float d0 = hA0 - hB0, d1 = hA1 - hB1, d2 = hA2 - hB2;
    const float s0 = hA0 + hB0, s1 = hA1 + hB1, s2 = hA2 + hB2;
    // the sign of theta: e . (nA x nB)
    const float c0 = A1 * B2 - A2 * B1, c1 = A2 * B0 - A0 * B2, c2 = A0 * B1 - A1 * B0;
    const float t = (e0 * c0 + e1 * c1) + e2 * c2;
    const float mag = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    const float psi = t >= 0.f ? mag : -mag;
    const float dpsi = .5f * sqrtf((s0 * s0 + s1 * s1) + s2 * s2);
    const float m_el = -(kc * (psi - psibar)) * dpsi;
    const float gA = le / AA, gB = le / BB;   // G2 = -gA nA, G3 = -gB nB
    const float re = 1.f / ee;
    const float wA = ((a0 * e0 + a1 * e1) + a2 * e2) * re, wB = ((b0 * e0 + b1 * e1) + b2 * e2) * re;
    const float uA = 1.f - wA, uB = 1.f - wB;
    const float nA[3] = {A0, A1, A2}, nB[3] = {B0, B1, B2};
    float m = m_el;
    if (MODE != 0) {
        float p2[3], p3[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float w1 = v[1][k] - v[0][k], w2 = v[2][k] - v[0][k], w3 = v[3][k] - v[0][k];
            p2[k] = w2 - wA * w1;
            p3[k] = w3 - wB * w1;
        }
        const float sA = (nA[0] * p2[0] + nA[1] * p2[1]) + nA[2] * p2[2];
        const float sB = (nB[0] * p3[0] + nB[1] * p3[1]) + nB[2] * p3[2];
        const float thetadot = -(gA * sA + gB * sB);
        const float psidot = dpsi * thetadot;
        const float bp = bkc * psidot;
        const float m_d = -bp * dpsi;
        const bool damped = bkc != 0.f;
        m = MODE == 2 ? (damped ? m_d : 0.f) : (damped ? m_el + m_d : m_el);
        *psidot_out = on ? psidot : 0.f;
        *power_out = on && damped ? bp * psidot : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f2 = m * -(gA * nA[k]), f3 = m * -(gB * nB[k]);
        const float f1 = -(wA * f2 + wB * f3), f0 = -(uA * f2 + uB * f3);
        rec[0][k] = on ? f0 : 0.f;
        rec[1][k] = on ? f1 : 0.f;
        rec[2][k] = on ? f2 : 0.f;
        rec[3][k] = on ? f3 : 0.f;
    }
    *psi_out = on ? psi : 0.f;
    return on;
}
MPM_SHELL_FN bool shell_hinge(const float x0[3], const float x1[3], const float x2[3], const float x3[3], float kc, float psibar,
                              float rec[4][3], float* psi_out) {
    return shell_hinge_core<0>(x0, x1, x2, x3, nullptr, kc, psibar, 0.f, rec, psi_out, nullptr, nullptr);
}
// The damped hinge: x[4][3], v[4][3]; with `elastic` false the damping part alone.  Returns psidot through psidot_out.
MPM_SHELL_FN bool shell_hinge_damped(const float (*x)[3], const float (*v)[3], float kc, float psibar, float bkc, float rec[4][3],
                                     float* psi_out, float* psidot_out, float* power_out, bool elastic = true) {
    return elastic ? shell_hinge_core<1>(x[0], x[1], x[2], x[3], v, kc, psibar, bkc, rec, psi_out, psidot_out, power_out)
                   : shell_hinge_core<2>(x[0], x[1], x[2], x[3], v, kc, psibar, bkc, rec, psi_out, psidot_out, power_out);
}

// shell_hinge's operations up to psi and dpsi, restated in the same order: psi and the gate are shell_hinge's bits.
// false: the hinge does not act (psi and dpsi are exact zeros).
MPM_SHELL_FN bool shell_angle(const float x0[3], const float x1[3], const float x2[3], const float x3[3], float* psi_out, float* dpsi_out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float e0 = x1[0] - x0[0], e1 = x1[1] - x0[1], e2 = x1[2] - x0[2];
    const float a0 = x2[0] - x0[0], a1 = x2[1] - x0[1], a2 = x2[2] - x0[2];
    const float b0 = x3[0] - x0[0], b1 = x3[1] - x0[1], b2 = x3[2] - x0[2];
    const float A0 = e1 * a2 - e2 * a1, A1 = e2 * a0 - e0 * a2, A2 = e0 * a1 - e1 * a0;
    const float B0 = b1 * e2 - b2 * e1, B1 = b2 * e0 - b0 * e2, B2 = b0 * e1 - b1 * e0;
    const float ee = (e0 * e0 + e1 * e1) + e2 * e2;
    const float AA = (A0 * A0 + A1 * A1) + A2 * A2;
    const float BB = (B0 * B0 + B1 * B1) + B2 * B2;
    const bool on = (ee >= SHELL_GATE) & (AA >= SHELL_GATE) & (BB >= SHELL_GATE);
    const float lA = sqrtf(AA), lB = sqrtf(BB);
    const float rA = 1.f / lA, rB = 1.f / lB;
    const float hA0 = A0 * rA, hA1 = A1 * rA, hA2 = A2 * rA;
    const float hB0 = B0 * rB, hB1 = B1 * rB, hB2 = B2 * rB;
    const float d0 = hA0 - hB0, d1 = hA1 - hB1, d2 = hA2 - hB2;
    const float s0 = hA0 + hB0, s1 = hA1 + hB1, s2 = hA2 + hB2;
    const float c0 = A1 * B2 - A2 * B1, c1 = A2 * B0 - A0 * B2, c2 = A0 * B1 - A1 * B0;
    const float t = (e0 * c0 + e1 * c1) + e2 * c2;
    const float mag = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    const float psi = t >= 0.f ? mag : -mag;
    const float dpsi = .5f * sqrtf((s0 * s0 + s1 * s1) + s2 * s2);
    *psi_out = on ? psi : 0.f;
    *dpsi_out = on ? dpsi : 0.f;
    return on;
}

// The return mapping of one hinge (the header, CREASES): the psibar the substep leaves, and whether the hinge yields.
// What a hinge that does not yield computes on the way (a division by dpsi = 0, a NaN) is never selected.
MPM_SHELL_FN float crease_return(float psi, float dpsi, bool on, float psibar, float y, float eta, float P, bool* yields_out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float d = psi - psibar;
    const float ad = fabsf(d);
    const float t = ad * dpsi;
    const bool yields = on && y > 0.f && t > y;
    const float dy = y / dpsi;
    const float dn = dy + eta * (ad - dy);
    const float pn = psi - copysignf(dn, d);
    *yields_out = yields;
    return yields ? fminf(fmaxf(pn, -P), P) : psibar;
}

// the hinge's energy term 1/2 kc (psi - psibar)^2, in float (the .w of plane 1)
MPM_SHELL_FN float shell_energy_term(float kc, float psibar, float psi) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float d = psi - psibar;
    return (.5f * kc) * (d * d);
}

}  // namespace mpm

#ifdef __HIPCC__
#include "mpm_step.h"

namespace mpm {

struct HingeArgs {
    const int4* ids;     // [hinge] particle ids (NfG + vertex) of x0, x1, x2, x3
    const float2* par;   // [hinge] (kc, psibar)
    float4* rec;         // [4][n] the corner records; .w: psi (plane 0), the energy term (1), 1 where the hinge acts (2),
                         // 1 where the hinge is cut (3)
    int n;
    const int2* faces;     // [hinge] faces A and B, GLOBAL original face ids (the cloth's first face + the cloth-local id)
    const uint8_t* torn;   // [n_faces] TearArgs::torn, set per launch (the header, CUT HINGES); nullptr: no hinge is cut
    int n_faces;           // what a face id is checked against before it indexes `torn`
    const float* bkc;      // [hinge] float(beta k cbar), set per launch (the header, HINGE DAMPING); nullptr: no damper
};
struct ShellArgs {
    const int* row_pid;          // [n_rows] particle id (NfG + vertex) of the row's vertex, ascending
    const unsigned* slice_off;   // [slices + 1] first record of a slice; its width is (next - this) / 64
    const unsigned* ent;         // records hinge << 2 | corner, SHELL_PAD: nothing
    int n_rows;
    const float4* rec;           // HingeArgs::rec
    int n_hinges;
};

// the four planes of hinge h from four positions (what k_hinge, k_hinge_eval and k_hinge_rest share); MODE != 0: and
// from four velocities and the hinge's bkc (shell_hinge_core); MODE 2: the .w of planes 0 and 1 are psidot and the power term
template <int MODE = 0>
MPM_DEV void hinge_store(const HingeArgs& a, int h, const float4 x[4], bool usable, bool cut = false, const float4* v = nullptr,
                         float bkc = 0.f) {
    const float2 q = a.par[h];
    const float X[4][3] = {{x[0].x, x[0].y, x[0].z}, {x[1].x, x[1].y, x[1].z}, {x[2].x, x[2].y, x[2].z}, {x[3].x, x[3].y, x[3].z}};
    float rec[4][3], psi, psidot = 0.f, power = 0.f;
    bool on;
    if (MODE == 0) {
        on = shell_hinge(X[0], X[1], X[2], X[3], q.x, q.y, rec, &psi) && usable;
    } else {
        const float V[4][3] = {{v[0].x, v[0].y, v[0].z}, {v[1].x, v[1].y, v[1].z}, {v[2].x, v[2].y, v[2].z}, {v[3].x, v[3].y, v[3].z}};
        on = shell_hinge_core<MODE>(X[0], X[1], X[2], X[3], V, q.x, q.y, bkc, rec, &psi, &psidot, &power) && usable;
    }
    const float w[4] = {on ? (MODE == 2 ? psidot : psi) : 0.f, on ? (MODE == 2 ? power : shell_energy_term(q.x, q.y, psi)) : 0.f,
                        on ? 1.f : 0.f, cut ? 1.f : 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        a.rec[(size_t)j * (size_t)a.n + (size_t)h] = on ? make_float4(rec[j][0], rec[j][1], rec[j][2], w[j]) : make_float4(0.f, 0.f, 0.f, j == 3 ? w[3] : 0.f);
}

// Whether hinge h is CUT on the flags `torn` (the header, CUT HINGES): the flags of its two faces, read by the ids fc of
// the host-built table.  An id outside [0, n_faces) is reported through `ok`, never used as an address, and cuts nothing.
// The two byte loads depend on the table alone, not on a slot or a position: a caller issues them beside its slot loads.
MPM_DEV bool hinge_cut(const uint8_t* torn, int n_faces, const int2& fc, bool& ok) {
    const bool ids = fc.x >= 0 && fc.x < n_faces && fc.y >= 0 && fc.y < n_faces;
    ok = ok && ids;
    const uint8_t ta = ids ? torn[fc.x] : (uint8_t)0, tb = ids ? torn[fc.y] : (uint8_t)0;
    return (ta | tb) != 0;
}

// Hinge h on the current positions.  Every index into a per-particle array comes through DP::imap from an id of the
// host-built table; an id outside the particle numbering or a slot that is no vertex slot is reported, never used as an
// address: the hinge's records are then exact zeros.
// While a.torn is set the hinge's two face ids come with the vertex ids (the first round trip) and the faces' two flags
// with the slots (the second): still three round trips of independent loads.
// MODE != 0 (the header, HINGE DAMPING): bkc comes with the ids and the four velocities with the four positions; a null
// a.bkc (k_hinge_eval<2> on an engine without the damper) is bkc = 0.
template <int MODE>
MPM_DEV void hinge_on_state(const DP& p, const PSet& S, const HingeArgs& a, int h, bool& bad) {
    const int4 id = a.ids[h];
    float bkc = 0.f;
    if (MODE != 0 && a.bkc) bkc = a.bkc[h];
    int2 fc = make_int2(0, 0);
    if (a.torn) fc = a.faces[h];
    const int c[4] = {id.x, id.y, id.z, id.w};
    int s[4];
    bool ok = true, cut = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) ok = ok && c[j] >= p.NfG && c[j] < p.NpG;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = ok ? p.imap[c[j]] : -1;
    if (a.torn) cut = hinge_cut(a.torn, a.n_faces, fc, ok);
#pragma unroll
    for (int j = 0; j < 4; ++j) ok = ok && s[j] >= p.Nf && s[j] < p.Np;
    float4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = ok ? S.q[0][s[j]] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v[4];
    if (MODE != 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ok ? S.q[1][s[j]] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    bad |= !ok;
    hinge_store<MODE>(a, h, x, ok && !cut, cut, v, bkc);
}

// Behind k_pressure (and k_vforce, k_bend, k_bend_damp, k_link) on the same stream, with the substep's DP: a substep that
// skips itself (and is run again by the host) writes nothing and adds nothing, so that the force is added once.
// MODE 0: no damper; MODE 1: while a cloth has beta > 0 (mpm_set_shell_damping), in its place.
template <int MODE>
__global__ __launch_bounds__(256) void k_hinge(DP p, HingeArgs a) {
    if (gated_out(p)) return;
    const int h = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (h < a.n) hinge_on_state<MODE>(p, p.set[p.ctl->cur], a, h, bad);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}
// mpm_shell_forces, mpm_shell_state: the same records without the gate (MODE 0: the elastic part alone, whatever the
// damper); mpm_shell_damping_forces, mpm_shell_damping_state: MODE 2, the damping part alone
template <int MODE>
__global__ __launch_bounds__(256) void k_hinge_eval(DP p, HingeArgs a) {
    const int h = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (h < a.n) hinge_on_state<MODE>(p, p.set[p.ctl->cur], a, h, bad);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}
// mpm_set_shell_bending: the same function on rest positions in original vertex order, pos[3 n_verts]; a.ids hold
// particle ids, `nfg` is taken off.  The host has checked every id.  What it leaves in plane 0's .w is psibar.
__global__ __launch_bounds__(256) void k_hinge_rest(HingeArgs a, const float* pos, int nfg, int n_verts) {
    const int h = (int)(blockIdx.x * 256 + threadIdx.x);
    if (h >= a.n) return;
    const int4 id = a.ids[h];
    const int c[4] = {id.x - nfg, id.y - nfg, id.z - nfg, id.w - nfg};
    bool ok = true;
    float4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok = ok && c[j] >= 0 && c[j] < n_verts;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float* q = pos + 3 * (size_t)(ok ? c[j] : 0);
        x[j] = make_float4(q[0], q[1], q[2], 0.f);
    }
    hinge_store(a, h, x, ok);
}

struct CreaseArgs {
    const int4* ids;    // HingeArgs::ids
    float2* par;        // HingeArgs::par of the same table: .y is the psibar in force, which k_crease owns
    const float4* cr;   // [hinge] (y, eta, P, psibar0) of the hinge's cloth and rest shape; nullptr: the tables do not exist
    int n;
    const int2* faces;     // HingeArgs::faces
    const uint8_t* torn;   // HingeArgs::torn, set per launch; nullptr: no hinge is cut
    int n_faces;
};

// Hinge h's psi, dpsi and the psibar the substep leaves, on the current positions: ids and psibar, slots, positions --
// three round trips of independent loads, the checks of hinge_on_state.  A bad id is reported, never used as an address,
// and the hinge then does not yield (psi = dpsi = 0, next = its psibar).  Returns whether the hinge yields.
// While a.torn is set, the face ids come with the vertex ids and the two flags with the slots, as in hinge_on_state; a
// CUT hinge loads no position: it does not yield and keeps its psibar (psi = dpsi = 0, next = its psibar).
MPM_DEV bool crease_on_state(const DP& p, const PSet& S, const CreaseArgs& a, int h, const float4& c, float& psi, float& dpsi,
                             float& next, bool& bad) {
    const int4 id = a.ids[h];
    const float psibar = a.par[h].y;
    int2 fc = make_int2(0, 0);
    if (a.torn) fc = a.faces[h];
    const int q[4] = {id.x, id.y, id.z, id.w};
    int s[4];
    bool ok = true, cut = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) ok = ok && q[j] >= p.NfG && q[j] < p.NpG;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = ok ? p.imap[q[j]] : -1;
    if (a.torn) cut = hinge_cut(a.torn, a.n_faces, fc, ok);
    if (cut) {
        bad |= !ok;
        psi = dpsi = 0.f;
        next = psibar;
        return false;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) ok = ok && s[j] >= p.Nf && s[j] < p.Np;
    float4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = ok ? S.q[0][s[j]] : make_float4(0.f, 0.f, 0.f, 0.f);
    bad |= !ok;
    const float X[4][3] = {{x[0].x, x[0].y, x[0].z}, {x[1].x, x[1].y, x[1].z}, {x[2].x, x[2].y, x[2].z}, {x[3].x, x[3].y, x[3].z}};
    const bool on = shell_angle(X[0], X[1], X[2], X[3], &psi, &dpsi) && ok;
    bool yields;
    next = crease_return(psi, dpsi, on, psibar, c.x, c.y, c.z, &yields);
    return yields;
}

// Immediately in front of k_hinge on the same stream, with the substep's DP, while the crease tables exist: one lane per
// hinge.  A hinge that yields gets its new psibar (one writer per hinge: a plain store), which k_hinge then reads; a
// substep that skips itself stores nothing.
__global__ __launch_bounds__(256) void k_crease(DP p, CreaseArgs a) {
    if (gated_out(p)) return;
    const int h = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (h < a.n) {
        const float4 c = a.cr[h];
        if (c.x != 0.f) {
            float psi, dpsi, next;
            if (crease_on_state(p, p.set[p.ctl->cur], a, h, c, psi, dpsi, next, bad)) a.par[h].y = next;
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}
// mpm_crease_measure: psi, dpsi and the psibar the substep would leave per hinge, without the gate and without the store
__global__ __launch_bounds__(256) void k_crease_eval(DP p, CreaseArgs a, float* psi_out, float* dpsi_out, float* next_out) {
    const int h = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (h < a.n) {
        float psi, dpsi, next;
        crease_on_state(p, p.set[p.ctl->cur], a, h, a.cr[h], psi, dpsi, next, bad);
        psi_out[h] = psi;
        dpsi_out[h] = dpsi;
        next_out[h] = next;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// Row r of the gather table: the records of the row's vertex, added in stored order.  A record that names no hinge of
// the table is reported and adds nothing.  false: the row's own vertex has no slot.
MPM_DEV bool shell_row(const DP& p, const ShellArgs& a, int r, int& s_out, float f[3], bool& bad) {
    const unsigned b0 = a.slice_off[r >> 6], b1 = a.slice_off[(r >> 6) + 1];
    const int width = (int)((b1 - b0) / SHELL_SLICE);
    const int s = p.imap[a.row_pid[r]];
    s_out = s;
    if (s < p.Nf || s >= p.Np) {
        bad = true;
        return false;
    }
    const unsigned* ent = a.ent + b0 + (r & 63);
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
    // SHELL_BATCH records at a time: the records, then the corner records they name -- two round trips of independent
    // loads per batch.  A record past the width loads nothing and enters as padding.
    for (int e0 = 0; e0 < width; e0 += SHELL_BATCH) {
        unsigned q[SHELL_BATCH];
        float4 g[SHELL_BATCH];
        bool live[SHELL_BATCH];
#pragma unroll
        for (int u = 0; u < SHELL_BATCH; ++u) {
            q[u] = SHELL_PAD;
            if (e0 + u < width) q[u] = ent[(size_t)(e0 + u) * SHELL_SLICE];
        }
#pragma unroll
        for (int u = 0; u < SHELL_BATCH; ++u) {
            const unsigned h = q[u] >> 2, j = q[u] & 3u;
            live[u] = q[u] != SHELL_PAD && h < (unsigned)a.n_hinges;
            bad |= q[u] != SHELL_PAD && !live[u];
            g[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live[u]) g[u] = a.rec[(size_t)j * (size_t)a.n_hinges + (size_t)h];
        }
#pragma unroll
        for (int u = 0; u < SHELL_BATCH; ++u)   // (in stored order; padding adds nothing)
            if (live[u]) {
                f0 += g[u].x;
                f1 += g[u].y;
                f2 += g[u].z;
            }
    }
    f[0] = f0; f[1] = f1; f[2] = f2;
    return true;
}

__global__ __launch_bounds__(256) void k_hinge_gather(DP p, ShellArgs a) {
    if (gated_out(p)) return;
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (shell_row(p, a, r, s, f, bad)) {
            p.f[0][s] += f[0];
            p.f[1][s] += f[1];
            p.f[2][s] += f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// mpm_shell_forces: out[3 (pid - NfG) ..] = the row's force (vertices without a row stay as the caller left them: zero)
__global__ __launch_bounds__(256) void k_hinge_gather_eval(DP p, ShellArgs a, float* out) {
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (shell_row(p, a, r, s, f, bad)) {
            float* o = out + 3 * (size_t)(a.row_pid[r] - p.NfG);
            o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

}  // namespace mpm
#endif  // __HIPCC__

namespace mpm {

// ---- host: the hinge list, the rest quantities, the gather table, the guard's rate ----------------------------------
struct ShellHinge {
    int32_t v[4];           // x0, x1, x2, x3 in the numbering of `idx`
    int32_t face_a, face_b; // face A (the lower id) and face B
};

// The hinges of the faces idx[3 n_faces] in ascending (min(v0, v1), max(v0, v1)): every edge shared by exactly two
// faces; x0 -> x1 as face A runs it.  The ids must be valid (the caller checks).
inline void mesh_hinges(const int32_t* idx, size_t n_faces, std::vector<ShellHinge>& out) {
    struct Side {
        int32_t u, v, from, to, w, face;   // edge (u < v), as the face runs it (from -> to), the vertex opposite, the face
    };
    std::vector<Side> sides;
    sides.reserve(3 * n_faces);
    for (size_t f = 0; f < n_faces; ++f)
        for (int c = 0; c < 3; ++c) {
            const int32_t a = idx[3 * f + c], b = idx[3 * f + (c + 1) % 3], w = idx[3 * f + (c + 2) % 3];
            sides.push_back(Side{std::min(a, b), std::max(a, b), a, b, w, (int32_t)f});
        }
    std::sort(sides.begin(), sides.end(), [](const Side& p, const Side& q) {
        return p.u != q.u ? p.u < q.u : (p.v != q.v ? p.v < q.v : p.face < q.face);
    });
    out.clear();
    for (size_t k = 0; k < sides.size();) {
        size_t m = k + 1;
        while (m < sides.size() && sides[m].u == sides[k].u && sides[m].v == sides[k].v) ++m;
        if (m - k == 2 && sides[k].u != sides[k].v) {
            const Side &A = sides[k], &B = sides[k + 1];
            out.push_back(ShellHinge{{A.from, A.to, A.w, B.w}, A.face, B.face});
        }
        k = m;
    }
}

// What the host needs of one hinge at a rest shape, in double from float positions
struct ShellRest {
    double cbar;        // 3 |e|^2 / (A_A + A_B)
    double dpsi;        // cos(theta / 2)
    double G[4];        // |G_j|
    int degenerate;     // 0: fine; 1: the edge has zero length; 2: face A has zero area; 3: face B
};
inline ShellRest shell_rest(const float* x0, const float* x1, const float* x2, const float* x3) {
    ShellRest r{};
    double e[3], a[3], b[3];
    for (int k = 0; k < 3; ++k) {
        e[k] = (double)x1[k] - (double)x0[k];
        a[k] = (double)x2[k] - (double)x0[k];
        b[k] = (double)x3[k] - (double)x0[k];
    }
    const double nA[3] = {e[1] * a[2] - e[2] * a[1], e[2] * a[0] - e[0] * a[2], e[0] * a[1] - e[1] * a[0]};
    const double nB[3] = {b[1] * e[2] - b[2] * e[1], b[2] * e[0] - b[0] * e[2], b[0] * e[1] - b[1] * e[0]};
    const double ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    const double lA = std::sqrt(nA[0] * nA[0] + nA[1] * nA[1] + nA[2] * nA[2]), lB = std::sqrt(nB[0] * nB[0] + nB[1] * nB[1] + nB[2] * nB[2]);
    const double areas = .5 * lA + .5 * lB;
    r.degenerate = !(ee > 0.0) || !std::isfinite(ee) ? 1 : (!(lA > 0.0) || !std::isfinite(lA) ? 2 : (!(lB > 0.0) || !std::isfinite(lB) ? 3 : 0));
    if (r.degenerate) return r;
    r.cbar = 3.0 * ee / areas;
    if (!std::isfinite(r.cbar)) {
        r.degenerate = 2;
        return r;
    }
    double s2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double s = nA[k] / lA + nB[k] / lB;
        s2 += s * s;
    }
    r.dpsi = .5 * std::sqrt(s2);
    const double le = std::sqrt(ee), gA = le / (lA * lA), gB = le / (lB * lB);
    const double wA = (a[0] * e[0] + a[1] * e[1] + a[2] * e[2]) / ee, wB = (b[0] * e[0] + b[1] * e[1] + b[2] * e[2]) / ee;
    double g0 = 0.0, g1 = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double G2 = -gA * nA[k], G3 = -gB * nB[k];
        const double G1 = -(wA * G2 + wB * G3), G0 = -((1.0 - wA) * G2 + (1.0 - wB) * G3);
        g0 += G0 * G0;
        g1 += G1 * G1;
    }
    r.G[0] = std::sqrt(g0);
    r.G[1] = std::sqrt(g1);
    r.G[2] = gA * lA;
    r.G[3] = gB * lB;
    return r;
}

// What mpm_set_shell_bending refuses before it looks at a mesh; empty: the numbers are fine
inline std::string shell_refusal(const ClothShell* t, size_t n) {
    for (size_t c = 0; c < n; ++c) {
        const std::string at = "shell bending: cloth " + std::to_string(c);
        if (!(std::isfinite(t[c].stiffness) && t[c].stiffness >= 0.f)) return at + ": the stiffness is negative or not finite";
        if (t[c].rest > SHELL_REST_FLAT) return at + ": unknown rest";
    }
    return std::string();
}

// mpm_set_creases: y, eta and P of every cloth from its ClothCrease, yep[3 c ..]; y and P are formed in double and rounded
// once, P of a cloth with max_angle 0 is 2.  The refusal in the caller's words, naming the cloth; empty: fine.
inline std::string crease_params(const ClothCrease* t, size_t n, float* yep) {
    // (max_angle may be pi as a float, which lies above pi: its chord still rounds to 2)
    const double pi = 3.14159265358979323846, pi_float = (double)3.14159274101257324f;
    for (size_t c = 0; c < n; ++c) {
        const std::string at = "creases: cloth " + std::to_string(c);
        const double ya = (double)t[c].yield_angle, ma = (double)t[c].max_angle;
        if (!(t[c].yield_angle == 0.f || (std::isfinite(ya) && ya > 0.0 && ya < pi))) return at + ": yield_angle is neither 0 nor in (0, pi)";
        if (!(t[c].hardening >= 0.f && t[c].hardening < 1.f)) return at + ": hardening is not in [0, 1)";
        if (!(t[c].max_angle == 0.f || (std::isfinite(ma) && ma > 0.0 && ma <= pi_float))) return at + ": max_angle is neither 0 nor in (0, pi]";
        const float y = t[c].yield_angle == 0.f ? 0.f : (float)(2.0 * std::sin(.5 * ya));
        if (t[c].yield_angle != 0.f && !(y > 0.f)) return at + ": yield_angle is too small, 2 sin(yield_angle / 2) rounds to 0";
        yep[3 * c] = y;
        yep[3 * c + 1] = t[c].hardening;
        yep[3 * c + 2] = t[c].max_angle == 0.f ? 2.f : (float)(2.0 * std::sin(.5 * ma));
    }
    return std::string();
}

// What mpm_set_shell_damping refuses before it looks at the hinges; empty: the numbers are fine
inline std::string shell_damping_refusal(const ClothShellDamping* t, size_t n) {
    for (size_t c = 0; c < n; ++c) {
        const std::string at = "shell damping: cloth " + std::to_string(c);
        if (!(std::isfinite(t[c].beta) && t[c].beta >= 0.f)) return at + ": beta is negative or not finite";
        if (!(t[c].reserved == 0.f)) return at + ": reserved must be 0";
    }
    return std::string();
}
// The damped guard's two rates (the header, HINGE DAMPING): row_rate[r] is the elastic guard's row sum over the row's mass,
// W their maximum over the rows that count (max_row_rate's rule), G the maximum of row_rate[r] beta[row_cloth[r]].
inline void shell_damped_rates(const std::vector<double>& row_rate, const std::vector<int>& row_cloth, const ClothShellDamping* t,
                               double* W, double* G) {
    double w = 0.0, g = 0.0;
    for (size_t r = 0; r < row_rate.size(); ++r)
        if (row_rate[r] > 0.0) {
            w = std::max(w, row_rate[r]);
            const double beta = (double)t[(size_t)row_cloth[r]].beta;
            if (beta > 0.0) g = std::max(g, row_rate[r] * beta);
        }
    *W = w;
    *G = g;
}

// The gather table of a hinge list: ids4 [4 n] vertex ids; row_vertex: the vertices with a row, ascending; nf: the faces in
// front.  A row's records are hinge << 2 | corner in ascending hinge id.  Needs no positions.
inline bool shell_rows(const int32_t* ids4, size_t n_hinges, const std::vector<int>& row_vertex, size_t nf, size_t slice,
                       RowTable<uint32_t>& out, std::string& why) {
    out = RowTable<uint32_t>{};
    const size_t n_rows = row_vertex.size();
    std::vector<std::vector<uint32_t>> rows(n_rows);
    for (size_t h = 0; h < n_hinges; ++h)
        for (int j = 0; j < 4; ++j) {
            const auto it = std::lower_bound(row_vertex.begin(), row_vertex.end(), (int)ids4[4 * h + j]);
            if (it == row_vertex.end() || *it != (int)ids4[4 * h + j]) {
                why = "shell bending: a hinge names a vertex without a row";
                return false;
            }
            rows[(size_t)(it - row_vertex.begin())].push_back((uint32_t)h << 2 | (uint32_t)j);
        }
    for (size_t r = 0; r < n_rows; ++r) out.row_pid.push_back((int)(nf + (size_t)row_vertex[r]));
    if (!sliced_ell(n_rows, slice, [&](size_t r) { return rows[r].size(); }, [&](size_t r, size_t q) { return rows[r][q]; },
                    [&](size_t) { return SHELL_PAD; }, out.slice_off, out.ent)) {
        why = "shell bending: the table is too large";
        return false;
    }
    return true;
}

// The tables of all cloths as the host lays them out (no device is touched)
struct ShellTable : RowTable<uint32_t> {   // the gather table: one row per vertex of the cloths with k > 0
    std::vector<int32_t> ids4;      // [4 hinge] vertex ids (0-based over all cloths) of x0, x1, x2, x3
    std::vector<float> kc;          // [hinge] float(k cbar)
    std::vector<double> cbar;       // [hinge] the rest shape's cbar (mpm_set_shell_damping: bkc = float(beta k cbar))
    std::vector<int> row_cloth;     // [row] its cloth
    std::vector<int> hinge_cloth;   // [hinge]
    std::vector<int32_t> faces2;    // [2 hinge] faces A and B as GLOBAL face ids: the cloth's first_face + the cloth-local id
    std::vector<int> row_vertex;    // [row] its vertex
    std::vector<double> rate_sum;   // [row] sum_h kc dpsibar^2 |Gbar_hi| sum_j |Gbar_hj| (the guard)
};

// cloths: anything with first_vertex, n_verts, first_face, n_faces; h_idx: the faces' vertex ids (0-based over all
// cloths); par: one ClothShell per cloth (stiffness 0: the cloth has no hinge and no row); shape: [3 n_verts] the
// positions that give cbar of every cloth (and the guard's geometry; for a cloth with MPM_SHELL_REST_FLAT the guard
// takes dpsibar = 1); nf: the faces in front; slice: rows per slice (SHELL_SLICE).  false with `why` set: a hinge of a cloth with k > 0 has a
// zero rest edge or a zero rest area (the face is named), or the tables do not fit.
template <class Cloth>
inline bool shell_table(const std::vector<Cloth>& cloths, const int* h_idx, size_t nf, const ClothShell* par, const float* shape,
                        size_t slice, ShellTable& out, std::string& why) {
    out = ShellTable{};
    for (size_t c = 0; c < cloths.size(); ++c) {
        if (!(par[c].stiffness > 0.f)) continue;
        const Cloth& cl = cloths[c];
        std::vector<ShellHinge> H;
        mesh_hinges(h_idx + 3 * cl.first_face, cl.n_faces, H);
        const size_t row0 = out.row_vertex.size();
        for (size_t v = 0; v < cl.n_verts; ++v) {
            out.row_vertex.push_back((int)(cl.first_vertex + v));
            out.rate_sum.push_back(0.0);
            out.row_cloth.push_back((int)c);
        }
        for (const ShellHinge& h : H) {
            const size_t id = out.kc.size();
            if (!(id < ((size_t)1 << 30) - 1)) {
                why = "shell bending: too many hinges";
                return false;
            }
            const ShellRest r = shell_rest(shape + 3 * (size_t)h.v[0], shape + 3 * (size_t)h.v[1], shape + 3 * (size_t)h.v[2],
                                           shape + 3 * (size_t)h.v[3]);
            if (r.degenerate) {
                const size_t face = cl.first_face + (size_t)(r.degenerate == 3 ? h.face_b : h.face_a);
                why = "shell bending: face " + std::to_string(face) +
                      (r.degenerate == 1 ? " has a hinge edge of zero rest length" : " has zero rest area");
                return false;
            }
            const float kc = (float)((double)par[c].stiffness * r.cbar);
            if (!std::isfinite(kc)) {
                why = "shell bending: face " + std::to_string(cl.first_face + (size_t)h.face_a) + ": k cbar is not a finite float";
                return false;
            }
            const double dpsi = par[c].rest == SHELL_REST_FLAT ? 1.0 : r.dpsi;
            const double gsum = ((r.G[0] + r.G[1]) + r.G[2]) + r.G[3];
            for (int j = 0; j < 4; ++j) {
                out.ids4.push_back(h.v[j]);
                const size_t row = row0 + ((size_t)h.v[j] - cl.first_vertex);
                out.rate_sum[row] += (double)kc * dpsi * dpsi * r.G[j] * gsum;
            }
            out.kc.push_back(kc);
            out.cbar.push_back(r.cbar);
            out.hinge_cloth.push_back((int)c);
            out.faces2.push_back((int32_t)(cl.first_face + (size_t)h.face_a));
            out.faces2.push_back((int32_t)(cl.first_face + (size_t)h.face_b));
        }
    }
    RowTable<uint32_t> rows;
    if (!shell_rows(out.ids4.data(), out.kc.size(), out.row_vertex, nf, slice, rows, why)) return false;
    static_cast<RowTable<uint32_t>&>(out) = rows;
    return true;
}

}  // namespace mpm
