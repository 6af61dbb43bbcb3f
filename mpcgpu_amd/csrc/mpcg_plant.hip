// mpcg_plant.hip — C ABI (include/mpcg.h) of the entries around the robot as data (mpcg_plant), one host path per call for float and double: the KKT block
// assembly (kkt_plant.hip.h), the merit function and the line-search step (merit_plant.hip.h, merit_plant_f32.hip.h), plant simulation
// and horizon shift (sim_plant.hip.h), inverse dynamics (invdyn_plant.hip.h).  Each kernel family is selected in ONE place — launch_kkt, launch_merit_points,
// simulate_impl — from the handle's options, the entry (the _xuref entries: COST >= 1) and the plant given (one with soft limits: COST = 2, saturating simulate).
#include <cmath>
#include <memory>
#include <type_traits>
#include "mpcg_handle.hpp"
#include "kkt_plant.hip.h"
#include "merit_plant.hip.h"
#include "merit_plant_f32.hip.h"
#include "sim_plant.hip.h"
#include "invdyn_plant.hip.h"

using namespace mpcg;

extern "C" {

// ---- the producer of the path's inputs: KKT block assembly with the robot as data (kkt_plant.hip.h) ----
struct mpcg_plant {
    int device = 0; PlantDev* d = nullptr; PlantDevT<float>* d32 = nullptr;      // (d32: the same tables rounded to float, behind d in ONE allocation)
    PlantDev host; PlantDevT<float> host32;                                      // what the device holds: mpcg_plant_clone_gravity copies these, mpcg_plant_get_gravity reads host.grav
    bool has_limits = false; mpcg_limits lim;                                    // mpcg_plant_clone_limits: the limits as given (host.xlo ... hold them for the kernels)
};

// `lim` into the tables of both precisions (the float ones rounded) and into pl->lim
static void plant_set_limits(mpcg_plant* pl, const mpcg_limits& lim) {
    pl->lim = lim;
    for (int i = 0; i < PJ; ++i) {
        pl->host.xlo[i] = lim.q_lo[i]; pl->host.xhi[i] = lim.q_hi[i]; pl->host.xlo[PJ + i] = lim.qd_lo[i]; pl->host.xhi[PJ + i] = lim.qd_hi[i];
        pl->host.ulo[i] = lim.u_lo[i]; pl->host.uhi[i] = lim.u_hi[i];
    }
    pl->host.limw[0] = lim.q_weight; pl->host.limw[1] = lim.qd_weight; pl->host.limw[2] = lim.u_weight;
    for (int i = 0; i < 2 * PJ; ++i) { pl->host32.xlo[i] = (float)pl->host.xlo[i]; pl->host32.xhi[i] = (float)pl->host.xhi[i]; }
    for (int i = 0; i < PJ; ++i) { pl->host32.ulo[i] = (float)pl->host.ulo[i]; pl->host32.uhi[i] = (float)pl->host.uhi[i]; }
    for (int i = 0; i < 3; ++i) pl->host32.limw[i] = (float)pl->host.limw[i];
}
// no bound on either side, zero weights, no flags: what a plant without limits holds and reports
static mpcg_limits no_limits() {
    mpcg_limits lim;
    for (int i = 0; i < PJ; ++i) {
        lim.q_lo[i] = lim.qd_lo[i] = lim.u_lo[i] = -INFINITY;
        lim.q_hi[i] = lim.qd_hi[i] = lim.u_hi[i] = INFINITY;
    }
    lim.q_weight = lim.qd_weight = lim.u_weight = 0.0;
    lim.flags = 0;
    return lim;
}

// pl->host and pl->host32 into ONE new allocation on pl->device (host32 behind host); on failure nothing stays allocated
static bool plant_upload(mpcg_plant* pl) {
    if (hipSetDevice(pl->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&pl->d), sizeof(PlantDev) + sizeof(PlantDevT<float>)) != hipSuccess) {
        pl->d = nullptr;
        return false;
    }
    if (hipMemcpy(pl->d, &pl->host, sizeof(PlantDev), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(pl->d + 1, &pl->host32, sizeof(PlantDevT<float>), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(pl->d);
        pl->d = nullptr;
        return false;
    }
    pl->d32 = reinterpret_cast<PlantDevT<float>*>(pl->d + 1);
    return true;
}

// A new plant for src's device with src's host tables and limits, nothing on the device yet (null: no memory).  The clone entries change one thing and
// upload; the owner frees the plant on any failure.  Clones, because kernels read the model through the constant address space as invariant data and
// captured graphs keep the pointer — a plant never changes after creation.
static std::unique_ptr<mpcg_plant> plant_clone(const mpcg_plant* src) {
    std::unique_ptr<mpcg_plant> pl(new (std::nothrow) mpcg_plant());
    if (pl) {
        pl->device = src->device;
        pl->host = src->host; pl->host32 = src->host32;
        pl->has_limits = src->has_limits; pl->lim = src->lim;
    }
    return pl;
}

int mpcg_plant_create(mpcg_plant** out, int device, uint32_t num_joints, const double* X_const, const double* I_spatial, const double* Xhom_const,
                      const int32_t* X_trig_idx, const double* X_trig_coef, const int32_t* X_trig_j, uint32_t n_X_trig,
                      const int32_t* Xhom_trig_idx, const double* Xhom_trig_coef, const int32_t* Xhom_trig_j, uint32_t n_Xhom_trig) {
    if (!out) return MPCG_ERR_INVALID;
    *out = nullptr;
    if (num_joints != (uint32_t)PJ) return fail(nullptr, MPCG_ERR_UNSUPPORTED, "mpcg_plant_create: the compiled specialisation has 7 joints (IIWA-14)");
    if (!X_const || !I_spatial || !Xhom_const || (n_X_trig && (!X_trig_idx || !X_trig_coef || !X_trig_j)) ||
        (n_Xhom_trig && (!Xhom_trig_idx || !Xhom_trig_coef || !Xhom_trig_j)))
        return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_create: null table");
    std::unique_ptr<PlantDev> hp(new (std::nothrow) PlantDev());
    if (!hp) return MPCG_ERR_NOMEM;
    memset(hp.get(), 0, sizeof(PlantDev));
    // The tables as given: X_k(q_k) = [[E, 0], [B, E]] with E = E0 + Es sin q_k + Ec cos q_k (likewise B), homogeneous transforms
    // R = R0 + Rs sin + Rc cos and translation p.  Tables are column-major (6x6 / 4x4), these are row-major 3x3 blocks.
    struct Given { double E0[PJ][9], Es[PJ][9], Ec[PJ][9], B0[PJ][9], Bs[PJ][9], Bc[PJ][9], R0[PJ][9], Rs[PJ][9], Rc[PJ][9], p[PJ][3], I[PJ][36]; };
    std::unique_ptr<Given> gv(new (std::nothrow) Given());
    if (!gv) return MPCG_ERR_NOMEM;
    memset(gv.get(), 0, sizeof(Given));
    auto place = [&](int k, int r, int c, double v, int which /*0 const, 1 sin, 2 cos*/) -> bool {
        double(*E)[9] = which == 0 ? gv->E0 : (which == 1 ? gv->Es : gv->Ec);
        double(*B)[9] = which == 0 ? gv->B0 : (which == 1 ? gv->Bs : gv->Bc);
        if (r < 3 && c < 3) { E[k][3 * r + c] = v; return true; }
        if (r >= 3 && c < 3) { B[k][3 * (r - 3) + c] = v; return true; }
        return v == 0.0 || (r >= 3 && c >= 3);             // upper-right block must be zero; lower-right repeats E
    };
    bool ok = true;
    for (int k = 0; k < PJ; ++k) {
        for (int c = 0; c < 6; ++c)
            for (int r = 0; r < 6; ++r) {
                ok = ok && place(k, r, c, X_const[k * 36 + c * 6 + r], 0);
                gv->I[k][6 * r + c] = I_spatial[k * 36 + c * 6 + r];
            }
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) gv->R0[k][3 * r + c] = Xhom_const[k * 16 + c * 4 + r];
        for (int r = 0; r < 3; ++r) gv->p[k][r] = Xhom_const[k * 16 + 12 + r];
    }
    for (uint32_t t = 0; t < n_X_trig && ok; ++t) {
        const int idx = X_trig_idx[t], k = idx / 36, c = (idx % 36) / 6, r = idx % 6, j = X_trig_j[t];
        if (idx < 0 || k >= PJ || j < 0 || j >= 2 * PJ || j % PJ != k) { ok = false; break; }     // joint k's transform depends on q_k only
        // a trig entry REPLACES the constant at that position (load_update_XImats_helpers overwrites it)
        place(k, r, c, 0.0, 0);
        ok = place(k, r, c, X_trig_coef[t], j < PJ ? 1 : 2);
    }
    for (uint32_t t = 0; t < n_Xhom_trig && ok; ++t) {
        const int idx = Xhom_trig_idx[t], k = idx / 16, c = (idx % 16) / 4, r = idx % 4, j = Xhom_trig_j[t];
        if (idx < 0 || k >= PJ || j < 0 || j >= 2 * PJ || j % PJ != k || r >= 3 || c >= 3) { ok = false; break; }
        gv->R0[k][3 * r + c] = 0.0;
        (j < PJ ? gv->Rs : gv->Rc)[k][3 * r + c] = Xhom_trig_coef[t];
    }
    if (!ok) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_create: tables do not describe a serial chain of revolute joints (X = [[E, 0], [B, E]], joint k depends on q_k)");
    // The kernel applies X_k(q) as blkdiag(Rz, Rz) Xtree, Rz = [[c, s, 0], [-s, c, 0], [0, 0, 1]] (a revolute joint about its own z axis,
    // the convention of GRiD's tables): row 0 = c T0 + s T1, row 1 = -s T0 + c T1, row 2 = T2 with T = E0 + Ec the transform at q = 0.
    // Verify that the given constant / sin / cos parts have exactly that form.
    double scale = 0.0;
    for (int k = 0; k < PJ; ++k)
        for (int e = 0; e < 9; ++e) {
            hp->ET[k][e] = gv->E0[k][e] + gv->Ec[k][e];
            hp->BT[k][e] = gv->B0[k][e] + gv->Bc[k][e];
            scale = fmax(scale, fmax(fabs(hp->ET[k][e]), fabs(hp->BT[k][e])));
        }
    auto rotz_form = [&](const double* T, const double* c0, const double* cs, const double* cc) {
        double worst = 0.0;
        for (int c = 0; c < 3; ++c) {
            worst = fmax(worst, fabs(cc[c] - T[c]) + fabs(cc[3 + c] - T[3 + c]) + fabs(cc[6 + c]));                 // cos part: rows 0, 1 of T
            worst = fmax(worst, fabs(cs[c] - T[3 + c]) + fabs(cs[3 + c] + T[c]) + fabs(cs[6 + c]));                 // sin part: T1, -T0
            worst = fmax(worst, fabs(c0[c]) + fabs(c0[3 + c]) + fabs(c0[6 + c] - T[6 + c]));                        // constant part: row 2
        }
        return worst;
    };
    double dev = 0.0;
    for (int k = 0; k < PJ; ++k) {
        dev = fmax(dev, rotz_form(hp->ET[k], gv->E0[k], gv->Es[k], gv->Ec[k]));
        dev = fmax(dev, rotz_form(hp->BT[k], gv->B0[k], gv->Bs[k], gv->Bc[k]));
    }
    if (!(dev <= 1e-12 * fmax(scale, 1.0)))
        return fail(nullptr, MPCG_ERR_UNSUPPORTED, "mpcg_plant_create: every joint must rotate about its own z axis, X_k(q) = blkdiag(Rz(q), Rz(q)) X_k(0) (the form of GRiD's tables)");
    // Spatial inertias: the kernel multiplies with the rigid-body form [[Ibar, skew(h)], [skew(h)^T, m 1]] (ten numbers).
    for (int k = 0; k < PJ; ++k) {
        const double* Ik = gv->I[k];
        double sc = 0.0, asym = 0.0;
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) { sc = fmax(sc, fabs(Ik[6 * r + c])); asym = fmax(asym, fabs(Ik[6 * r + c] - Ik[6 * c + r])); }
        if (!(asym <= 1e-12 * fmax(1.0, sc))) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_create: spatial inertias must be symmetric");
        const double mass = Ik[6 * 3 + 3], h[3] = {Ik[6 * 2 + 4], Ik[6 * 0 + 5], Ik[6 * 1 + 3]};      // skew(h) = [[0, -hz, hy], [hz, 0, -hx], [-hy, hx, 0]]
        const double sk[9] = {0, -h[2], h[1], h[2], 0, -h[0], -h[1], h[0], 0};
        double devI = 0.0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                devI = fmax(devI, fabs(Ik[6 * r + 3 + c] - sk[3 * r + c]));
                devI = fmax(devI, fabs(Ik[6 * (3 + r) + 3 + c] - (r == c ? mass : 0.0)));
            }
        if (!(devI <= 1e-12 * fmax(1.0, sc)))
            return fail(nullptr, MPCG_ERR_UNSUPPORTED, "mpcg_plant_create: spatial inertias must have the rigid-body form [[Ibar, skew(m c)], [skew(m c)^T, m 1]]");
        const double ib[10] = {Ik[0], Ik[1], Ik[2], Ik[7], Ik[8], Ik[14], h[0], h[1], h[2], mass};
        memcpy(hp->Ib[k], ib, sizeof(ib));
    }
    // The end-effector position and Jacobian come out of the spatial transforms on the device (kkt_plant.hip.h, round 0); the reference
    // takes them from the homogeneous transforms.  Both tables describe the same chain: check it at three configurations.
    {
        const double qs[3][PJ] = {{0, 0, 0, 0, 0, 0, 0}, {0.3, -0.7, 1.1, 0.5, -1.3, 0.9, 0.2}, {-2.1, 1.4, -0.6, 1.9, 0.8, -1.7, 2.5}};
        double worst = 0.0;
        for (int t = 0; t < 3; ++t) {
            double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pos[3] = {0, 0, 0};
            double W[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, V[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};       // motion vectors [e_i; 0] pushed through the chain
            for (int k = 0; k < PJ; ++k) {
                const double sn = sin(qs[t][k]), cs = cos(qs[t][k]);
                double H[9], Rn[9];
                for (int e = 0; e < 9; ++e) H[e] = gv->R0[k][e] + gv->Rs[k][e] * sn + gv->Rc[k][e] * cs;
                for (int r = 0; r < 3; ++r) {
                    pos[r] += R[3 * r] * gv->p[k][0] + R[3 * r + 1] * gv->p[k][1] + R[3 * r + 2] * gv->p[k][2];
                    for (int c = 0; c < 3; ++c) Rn[3 * r + c] = R[3 * r] * H[c] + R[3 * r + 1] * H[3 + c] + R[3 * r + 2] * H[6 + c];
                }
                memcpy(R, Rn, sizeof(R));
                for (int i = 0; i < 3; ++i) {
                    double tw[3], tu[3];
                    for (int r = 0; r < 3; ++r) {
                        tw[r] = hp->ET[k][3 * r] * W[i][0] + hp->ET[k][3 * r + 1] * W[i][1] + hp->ET[k][3 * r + 2] * W[i][2];
                        tu[r] = hp->BT[k][3 * r] * W[i][0] + hp->BT[k][3 * r + 1] * W[i][1] + hp->BT[k][3 * r + 2] * W[i][2] +
                                hp->ET[k][3 * r] * V[i][0] + hp->ET[k][3 * r + 1] * V[i][1] + hp->ET[k][3 * r + 2] * V[i][2];
                    }
                    W[i][0] = cs * tw[0] + sn * tw[1]; W[i][1] = cs * tw[1] - sn * tw[0]; W[i][2] = tw[2];
                    V[i][0] = cs * tu[0] + sn * tu[1]; V[i][1] = cs * tu[1] - sn * tu[0]; V[i][2] = tu[2];
                }
            }
            const double ee[3] = {-(W[2][0] * V[1][0] + W[2][1] * V[1][1] + W[2][2] * V[1][2]), W[2][0] * V[0][0] + W[2][1] * V[0][1] + W[2][2] * V[0][2],
                                  -(W[1][0] * V[0][0] + W[1][1] * V[0][1] + W[1][2] * V[0][2])};
            for (int r = 0; r < 3; ++r) worst = fmax(worst, fabs(ee[r] - pos[r]));
        }
        if (!(worst <= 1e-9))
            return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_create: the homogeneous transforms (Xhom) and the spatial transforms (X) describe different chains");
    }
    gv.reset();
    std::unique_ptr<mpcg_plant> pl(new (std::nothrow) mpcg_plant());
    if (!pl) return MPCG_ERR_NOMEM;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return fail(nullptr, MPCG_ERR_HIP, "mpcg_plant_create: no HIP device");
    pl->device = device;
    // the float build of the kernel (linsys_t's own arithmetic, "kkt_f32") reads the same tables rounded to float
    std::unique_ptr<PlantDevT<float>> hp32(new (std::nothrow) PlantDevT<float>());
    if (!hp32) return MPCG_ERR_NOMEM;
    for (int k = 0; k < PJ; ++k) {
        for (int e = 0; e < 9; ++e) { hp32->ET[k][e] = (float)hp->ET[k][e]; hp32->BT[k][e] = (float)hp->BT[k][e]; }
        for (int e = 0; e < 10; ++e) hp32->Ib[k][e] = (float)hp->Ib[k][e];
    }
    pl->host = *hp; pl->host32 = *hp32;                     // (grav = {0, 0, 0}: hp was zero-filled, hp32 value-initialised)
    plant_set_limits(pl.get(), no_limits());
    if (!plant_upload(pl.get())) return fail(nullptr, MPCG_ERR_HIP, "mpcg_plant_create: cannot place the model on the device");
    *out = pl.release();
    return MPCG_OK;
}

// The KUKA LBR iiwa 14 the reference is built for, from the tables compiled into the library (csrc/iiwa14_model.inc): what
// gato_plant::initializeDynamicsConstMem<T>() returns in the reference (include/dynamics/iiwa/iiwa_eepos_plant.cuh:63-66).
#include "iiwa14_model.inc"
int mpcg_plant_create_iiwa14(mpcg_plant** out, int device) {
    return mpcg_plant_create(out, device, 7, kIiwa14_X_const, kIiwa14_I, kIiwa14_Xhom_const, kIiwa14_X_trig_idx, kIiwa14_X_trig_coef, kIiwa14_X_trig_j,
                             (uint32_t)(sizeof(kIiwa14_X_trig_idx) / sizeof(int32_t)), kIiwa14_Xhom_trig_idx, kIiwa14_Xhom_trig_coef, kIiwa14_Xhom_trig_j,
                             (uint32_t)(sizeof(kIiwa14_Xhom_trig_idx) / sizeof(int32_t)));
}

// The plant with another root acceleration (PlantDevT::grav): a NEW plant with its own device allocation (plant_clone).
int mpcg_plant_clone_gravity(mpcg_plant** out, const mpcg_plant* src, const double base_accel[3]) {
    if (!out) return MPCG_ERR_INVALID;
    *out = nullptr;
    if (!src || !base_accel) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_clone_gravity: null argument");
    if (!std::isfinite(base_accel[0]) || !std::isfinite(base_accel[1]) || !std::isfinite(base_accel[2]))
        return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_clone_gravity: base_accel must be finite");
    std::unique_ptr<mpcg_plant> pl = plant_clone(src);      // (a gravity clone of a limits plant keeps its limits)
    if (!pl) return MPCG_ERR_NOMEM;
    for (int r = 0; r < 3; ++r) {
        pl->host.grav[r] = base_accel[r] + 0.0;             // (-0 becomes +0: a zero vector is the plain plant's, whatever its sign bits)
        pl->host32.grav[r] = (float)pl->host.grav[r];
    }
    if (!plant_upload(pl.get())) return fail(nullptr, MPCG_ERR_HIP, "mpcg_plant_clone_gravity: cannot place the model on the device");
    *out = pl.release();
    return MPCG_OK;
}

int mpcg_plant_get_gravity(const mpcg_plant* p, double out[3]) {
    if (!p || !out) return MPCG_ERR_INVALID;
    for (int r = 0; r < 3; ++r) out[r] = p->host.grav[r];
    return MPCG_OK;
}

// The plant with soft limits (PlantDevT::xlo ..., mpcg_limits): a NEW plant for the reasons mpcg_plant_clone_gravity gives; the gravity of src is kept.
int mpcg_plant_clone_limits(mpcg_plant** out, const mpcg_plant* src, const mpcg_limits* lim) {
    static_assert(PJ == 7, "mpcg_limits holds seven joints");
    if (!out) return MPCG_ERR_INVALID;
    *out = nullptr;
    if (!src || !lim) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_clone_limits: null argument");
    const double* lo[3] = {lim->q_lo, lim->qd_lo, lim->u_lo};
    const double* hi[3] = {lim->q_hi, lim->qd_hi, lim->u_hi};
    for (int t = 0; t < 3; ++t)
        for (int i = 0; i < PJ; ++i) {
            if (std::isnan(lo[t][i]) || std::isnan(hi[t][i])) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_clone_limits: a bound is NaN");
            if (lo[t][i] > hi[t][i]) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_clone_limits: a lower bound exceeds its upper bound");
            if (lo[t][i] == INFINITY || hi[t][i] == -INFINITY)
                return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_clone_limits: a lower bound of +inf or an upper bound of -inf");
        }
    const double w[3] = {lim->q_weight, lim->qd_weight, lim->u_weight};
    for (int t = 0; t < 3; ++t)
        if (!std::isfinite(w[t]) || w[t] < 0.0) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_clone_limits: weights must be finite and >= 0");
    if (lim->flags & ~MPCG_LIMITS_SIM_SATURATE) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_plant_clone_limits: unknown flag bit");
    std::unique_ptr<mpcg_plant> pl = plant_clone(src);
    if (!pl) return MPCG_ERR_NOMEM;
    pl->has_limits = true;
    plant_set_limits(pl.get(), *lim);
    if (!plant_upload(pl.get())) return fail(nullptr, MPCG_ERR_HIP, "mpcg_plant_clone_limits: cannot place the model on the device");
    *out = pl.release();
    return MPCG_OK;
}

int mpcg_plant_get_limits(const mpcg_plant* p, mpcg_limits* out, int* has_limits) {
    if (!p || !out || !has_limits) return MPCG_ERR_INVALID;
    *out = p->lim;
    *has_limits = p->has_limits ? 1 : 0;
    return MPCG_OK;
}

int mpcg_plant_destroy(mpcg_plant* p) {
    if (p && p->d) { RelaxedCaptureScope relaxed; (void)hipSetDevice(p->device); (void)hipFree(p->d); }
    delete p;
    return MPCG_OK;
}

// mpcg_generate_kkt (T = float) and mpcg_generate_kkt_f64 (T = double): one host path (fn: the entry point's name).  "kkt_f32" selects a build of the float entry only.
// The _xuref entries (xuref = true) go the same way with the COST = 1 instantiation of the build the options select; `ref` is copied into the launch.
extern "C++" {
// the rules of mpcg_xuref (include/mpcg.h); MPCG_OK, or the error left in the handle
static int check_xuref(mpcg_handle* h, const char* fn, const mpcg_xuref* ref, const void* d_eePos_traj) {
    static_assert(XUREF_QD_RELATIVE == MPCG_XUREF_QD_RELATIVE && XUREF_U_RELATIVE == MPCG_XUREF_U_RELATIVE, "the flags of the header");
    const std::string who(fn);
    if (!ref || !ref->d_xu_traj) return fail(h, MPCG_ERR_INVALID, who + ": null mpcg_xuref or d_xu_traj");
    if (ref->traj_steps == 0 || (ref->traj_batch_stride != 0 && ref->traj_batch_stride < ref->traj_steps))
        return fail(h, MPCG_ERR_INVALID, who + ": needs traj_steps >= 1 and traj_batch_stride 0 or >= traj_steps");
    if (!std::isfinite(ref->ee_cost) || !std::isfinite(ref->q_cost) || ref->ee_cost < 0.0 || ref->q_cost < 0.0)
        return fail(h, MPCG_ERR_INVALID, who + ": ee_cost and q_cost must be finite and >= 0");
    if (ref->flags & ~(MPCG_XUREF_QD_RELATIVE | MPCG_XUREF_U_RELATIVE)) return fail(h, MPCG_ERR_INVALID, who + ": unknown flag bit");
    if (!d_eePos_traj && ref->ee_cost != 0.0) return fail(h, MPCG_ERR_INVALID, who + ": d_eePos_traj may be NULL only if ee_cost is 0");
    return MPCG_OK;
}

// What the entries that take a plant check once their own pointers are good (fn: the entry's name), in the order each of them always has: 14 x 7 only, plant
// and handle on one device and, where the entry cannot honour them (the plain KKT and merit entries: the two families differ in the last block's quirk, and a
// silent switch would change numbers), a plant without limits.  MPCG_OK, or the error left in the handle.  Checks that an entry makes between these and
// its batch checks stay in the entry, and so do the batch checks: every pair of wrong arguments is answered as it always was.
static int check_plant(mpcg_handle* h, const char* fn, const mpcg_plant* plant, uint32_t control_size, bool honours_limits) {
    if (control_size != (uint32_t)PJ || h->n != 2u * PJ) return fail(h, MPCG_ERR_UNSUPPORTED, std::string(fn) + ": state_size 14 / control_size 7 (IIWA-14) only");
    if (plant->device != h->device) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": plant and handle live on different devices");
    if (!honours_limits && plant->has_limits)
        return fail(h, MPCG_ERR_UNSUPPORTED, std::string(fn) + ": the plant has limits (mpcg_plant_clone_limits), which only the _xuref entries honour: call " + fn +
                                                 "'s _xuref twin with the neutral cost (ee_cost = 1, q_cost = 0, no flags)");
    return MPCG_OK;
}

template <typename S, typename T>
static XuRefT<S, T> xuref_args(const mpcg_xuref* ref) {
    XuRefT<S, T> x;
    x.xu_traj = static_cast<const T*>(ref->d_xu_traj); x.traj_offset = ref->d_traj_offset; x.traj_steps = ref->traj_steps; x.traj_stride = ref->traj_batch_stride;
    x.ee_cost = (S)ref->ee_cost; x.q_cost = (S)ref->q_cost; x.flags = ref->flags;
    return x;
}

// One launch of generate_kkt_kernel<ANALYTIC, R, *, T, COST>: the argument struct that instantiation takes (KktArgsSel) from the filled KktArgsT — with the plan's
// when COST >= 1 — and the explicit or the semi-implicit instantiation ("integrator"; a compile-time parameter: the explicit ones are the kernels they were).
template <bool ANALYTIC, typename R, typename T, int COST, typename S>
static void launch_kkt(bool semi, long blocks, hipStream_t st, const KktArgsT<S, T>& base, const mpcg_xuref* ref) {
    static_assert(std::is_same<S, typename KktR<R>::scalar>::value, "the arithmetic of the build");
    typename KktArgsSel<COST, S, T>::type a;
    static_cast<KktArgsT<S, T>&>(a) = base;
    if constexpr (COST >= 1) a.ref = xuref_args<S, T>(ref);
    hipLaunchKernelGGL((semi ? generate_kkt_kernel<ANALYTIC, R, 1, T, COST> : generate_kkt_kernel<ANALYTIC, R, 0, T, COST>), dim3((unsigned)blocks), dim3(KKT_THREADS), 0, st, a);
}

template <typename T>
static int generate_kkt_impl(mpcg_handle* h, const char* fn, const mpcg_plant* plant, uint32_t control_size, T timestep, const T* d_eePos_traj,
                             const T* d_xs, const T* d_xu, T qd_cost, T r_cost, T* d_G_dense, T* d_C_dense, T* d_g, T* d_c, uint32_t batch, void* stream,
                             bool xuref = false, const mpcg_xuref* ref = nullptr) {
    if (!h || !plant) return MPCG_ERR_INVALID;
    if ((!d_eePos_traj && !xuref) || !d_xs || !d_xu || !d_G_dense || !d_C_dense || !d_g || !d_c)
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    if (xuref) { const int rc = check_xuref(h, fn, ref, d_eePos_traj); if (rc != MPCG_OK) return rc; }
    { const int rc = check_plant(h, fn, plant, control_size, xuref); if (rc != MPCG_OK) return rc; }
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    auto fill = [&](auto& k, const auto* tables) {        // one fill for either arithmetic: the scalars convert to the struct's S
        k.plant = tables; k.eePos_traj = d_eePos_traj; k.xs = d_xs; k.xu = d_xu;
        k.G = d_G_dense; k.C = d_C_dense; k.g = d_g; k.c = d_c;
        k.N = (int)h->N; k.batch = (int)batch; k.dt = timestep; k.qd_cost = qd_cost; k.r_cost = r_cost;
        k.analytic = h->kkt_analytic;
    };
    // one wavefront per `items` (trajectory, knot) pairs — KKT_ITEMS, the packed build 2 KKT_ITEMS — and at most 32 per CU: the kernels loop
    auto grid = [&](long items) { return std::min(((long)batch * (h->N - 1) + items - 1) / items, (long)h->num_cus * 32); };
    const bool semi = h->integrator == 1;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // The build, from the handle's options and T, for the COST the call has.  Float arrays: "kkt_f32" (with the analytic route only) is linsys_t = float
    // arithmetic throughout, as the reference's GRiD code, on the tables rounded to float — 1: two knots per lane in packed float (whatever the size of the
    // call: a trajectory's results do not depend on what else is in the batch); 2: one knot per lane (the packed build's checker; 8 % faster than the
    // default, where the packed build is 1.6x faster on throughput-sized calls).  Otherwise, and for double arrays always: float64 inside, either gradient route.
    auto launch = [&](auto cost) {
        constexpr int COST = decltype(cost)::value;
        if constexpr (std::is_same<T, float>::value) {
            if (h->kkt_analytic && h->kkt_f32) {
                KktArgsT<float> f;
                fill(f, plant->d32);
                if (h->kkt_f32 == 1) return launch_kkt<true, kkt_f2, float, COST>(semi, grid(2 * KKT_ITEMS), st, f, ref);
                return launch_kkt<true, float, float, COST>(semi, grid(KKT_ITEMS), st, f, ref);
            }
        }
        KktArgsT<double, T> a;
        fill(a, plant->d);
        if (h->kkt_analytic) return launch_kkt<true, double, T, COST>(semi, grid(KKT_ITEMS), st, a, ref);
        return launch_kkt<false, double, T, COST>(semi, grid(KKT_ITEMS), st, a, ref);
    };
    // COST = 0: the end-effector plant's cost; the _xuref entries: 1, and 2 exactly when the plant given has limits
    if (!xuref) launch(std::integral_constant<int, 0>());
    else if (plant->has_limits) launch(std::integral_constant<int, 2>());
    else launch(std::integral_constant<int, 1>());
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}
}  // extern "C++"

int mpcg_generate_kkt(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, float timestep, const float* d_eePos_traj,
                      const float* d_xs, const float* d_xu, float qd_cost, float r_cost, float* d_G_dense, float* d_C_dense,
                      float* d_g, float* d_c, uint32_t batch, void* stream) {
    return generate_kkt_impl<float>(h, "mpcg_generate_kkt", plant, control_size, timestep, d_eePos_traj, d_xs, d_xu, qd_cost, r_cost, d_G_dense, d_C_dense, d_g, d_c, batch, stream);
}

int mpcg_generate_kkt_f64(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, double timestep, const double* d_eePos_traj,
                          const double* d_xs, const double* d_xu, double qd_cost, double r_cost, double* d_G_dense, double* d_C_dense,
                          double* d_g, double* d_c, uint32_t batch, void* stream) {
    return generate_kkt_impl<double>(h, "mpcg_generate_kkt_f64", plant, control_size, timestep, d_eePos_traj, d_xs, d_xu, qd_cost, r_cost, d_G_dense, d_C_dense, d_g, d_c, batch, stream);
}

int mpcg_generate_kkt_xuref(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, float timestep, const float* d_eePos_traj,
                            const float* d_xs, const float* d_xu, float qd_cost, float r_cost, const mpcg_xuref* ref, float* d_G_dense, float* d_C_dense,
                            float* d_g, float* d_c, uint32_t batch, void* stream) {
    return generate_kkt_impl<float>(h, "mpcg_generate_kkt_xuref", plant, control_size, timestep, d_eePos_traj, d_xs, d_xu, qd_cost, r_cost, d_G_dense, d_C_dense, d_g, d_c, batch,
                                    stream, true, ref);
}

int mpcg_generate_kkt_xuref_f64(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, double timestep, const double* d_eePos_traj,
                                const double* d_xs, const double* d_xu, double qd_cost, double r_cost, const mpcg_xuref* ref, double* d_G_dense, double* d_C_dense,
                                double* d_g, double* d_c, uint32_t batch, void* stream) {
    return generate_kkt_impl<double>(h, "mpcg_generate_kkt_xuref_f64", plant, control_size, timestep, d_eePos_traj, d_xs, d_xu, qd_cost, r_cost, d_G_dense, d_C_dense, d_g, d_c,
                                     batch, stream, true, ref);
}

// ---- merit function and line search (merit_plant.hip.h): one host path per call for the float entries (T = float) and their _f64 twins (T = double) ----
extern "C++" {
template <typename T>
static int check_steps(mpcg_handle* h, const char* who, const T* step_sizes, uint32_t num_steps) {
    if (!step_sizes) return fail(h, MPCG_ERR_INVALID, std::string(who) + ": null step_sizes");
    if (num_steps == 0 || num_steps > (uint32_t)MPCG_MAX_STEP_SIZES) return fail(h, MPCG_ERR_INVALID, std::string(who) + ": num_steps must be 1..16 (MPCG_MAX_STEP_SIZES)");
    return MPCG_OK;
}

// One launch of the point-merit kernel of the arithmetic S — double: merit_points_kernel<T, *, COST>; float: the packed merit_points_f32_kernel<*, COST> (float
// arrays only) — with the argument struct that instantiation takes (MeritArgsSel) from the filled MeritArgsT, the plan's added when COST >= 1.
template <int COST, typename T, typename S>
static void launch_merit_points(bool semi, long blocks, hipStream_t st, const MeritArgsT<T, S>& base, const mpcg_xuref* ref) {
    typename MeritArgsSel<COST, T, S>::type a;
    static_cast<MeritArgsT<T, S>&>(a) = base;
    if constexpr (COST >= 1) a.ref = xuref_args<S, T>(ref);
    if constexpr (std::is_same<S, float>::value)
        hipLaunchKernelGGL((semi ? merit_points_f32_kernel<1, COST> : merit_points_f32_kernel<0, COST>), dim3((unsigned)blocks), dim3(KKT_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((semi ? merit_points_kernel<T, 1, COST> : merit_points_kernel<T, 0, COST>), dim3((unsigned)blocks), dim3(KKT_THREADS), 0, st, a);
}

template <typename T>
static int compute_merit_impl(mpcg_handle* h, const char* fn, const mpcg_plant* plant, uint32_t control_size, T timestep, const T* d_eePos_traj, const T* d_xs,
                              const T* d_xu, const T* d_dz, const T* step_sizes, uint32_t num_steps, T mu, T qd_cost, T r_cost, T* d_merit, uint32_t batch, void* stream,
                              bool xuref = false, const mpcg_xuref* ref = nullptr) {
    static_assert(MERIT_MAX_STEPS == MPCG_MAX_STEP_SIZES, "scratch row stride");
    if (!h || !plant) return MPCG_ERR_INVALID;
    if ((!d_eePos_traj && !xuref) || !d_xu || !d_merit) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    if (xuref) { const int rc = check_xuref(h, fn, ref, d_eePos_traj); if (rc != MPCG_OK) return rc; }
    { const int rc = check_steps(h, fn, step_sizes, num_steps); if (rc != MPCG_OK) return rc; }
    { const int rc = check_plant(h, fn, plant, control_size, xuref); if (rc != MPCG_OK) return rc; }
    T alpha[MERIT_MAX_STEPS];
    bool moved = false;
    for (uint32_t i = 0; i < (uint32_t)MERIT_MAX_STEPS; ++i) { alpha[i] = i < num_steps ? step_sizes[i] : T(0); moved = moved || alpha[i] != T(0); }
    if (moved && !d_dz) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": d_dz may be NULL only if every step size is 0");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the point merits: made at the first call (not stream-ordered: hipMalloc), shared by the four entries
    { const int rc = buf_reserve(h, BUF_MERIT, (size_t)h->max_batch * MERIT_MAX_STEPS * h->N * sizeof(double), &st, fn); if (rc != MPCG_OK) return rc; }
    double* const points = h->ptr<double>(BUF_MERIT);
    auto fill = [&](auto& k, const auto* tables) {        // one fill for either arithmetic: the scalars convert to the struct's S
        k.plant = tables; k.eePos_traj = d_eePos_traj; k.xs = d_xs; k.xu = d_xu; k.dz = d_dz; k.point = points;
        k.N = (int)h->N; k.batch = (int)batch; k.A = (int)num_steps;
        k.dt = timestep; k.mu = mu; k.qd_cost = qd_cost; k.r_cost = r_cost;
        memcpy(k.alpha, alpha, sizeof(alpha));
    };
    const long items = (long)batch * num_steps * h->N;     // (trajectory, step size, knot)
    const bool semi = h->integrator == 1;          // "integrator": the map mpcg_generate_kkt linearised (one knob for both, every build)
    // The build, for the COST the call has.  Float arrays with "merit_f32": the reference's own arithmetic (merit.cuh, T = float), two items per lane group in
    // packed float, whatever the size of the call.  Otherwise, and for double arrays always: float64 inside.
    auto launch = [&](auto cost) -> int {
        constexpr int COST = decltype(cost)::value;
        if constexpr (std::is_same<T, float>::value) {
            if (h->merit_f32) {
                MeritArgsT<float, float> f;
                fill(f, plant->d32);
                // one wavefront per trip of 2 KKT_ITEMS items (no trip loop: merit_plant_f32.hip.h); at most max_batch x 16 x N / 8 of them, and a handle whose
                // scratch of max_batch x 16 x N doubles could be allocated stays far below the 2^31 - 1 workgroups a grid dimension holds
                const long pblocks = (items + 2 * KKT_ITEMS - 1) / (2 * KKT_ITEMS);
                if (pblocks > 0x7fffffffL) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch x num_steps x knot_points exceeds the grid");
                launch_merit_points<COST>(semi, pblocks, st, f, ref);
                return MPCG_OK;
            }
        }
        MeritArgsT<T> a;
        fill(a, plant->d);
        // one wavefront per KKT_ITEMS items and at most 32 per CU: the kernel loops
        launch_merit_points<COST>(semi, std::min((items + KKT_ITEMS - 1) / KKT_ITEMS, (long)h->num_cus * 32), st, a, ref);
        return MPCG_OK;
    };
    // COST as in generate_kkt_impl: 0; the _xuref entries 1, and 2 exactly when the plant given has limits
    const int rc = !xuref ? launch(std::integral_constant<int, 0>()) : plant->has_limits ? launch(std::integral_constant<int, 2>()) : launch(std::integral_constant<int, 1>());
    if (rc != MPCG_OK) return rc;
    HIP_TRY(h, hipGetLastError());
    const int rows = (int)(batch * num_steps);             // the row sums, stored as T
    hipLaunchKernelGGL(merit_sum_kernel<T>, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, points, d_merit, (int)h->N, (int)num_steps, rows);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

// mpcg_line_search_step(_f64) and mpcg_line_search_step_rho(_f64): one host path (fn: the entry point's name; rho: null for the former)
template <typename T>
static int line_search_step_impl(mpcg_handle* h, const char* fn, uint32_t control_size, const T* d_merit, const T* step_sizes, uint32_t num_steps,
                                 T* d_merit_ref, const T* d_dz, T* d_xu, int32_t* d_step, const StepRhoArgsT<T>* rho, uint32_t batch, void* stream) {
    typedef StepArgsT<T> Plain;
    typedef StepRhoArgsT<T> WithRho;
    if (!h) return MPCG_ERR_INVALID;
    if (!d_merit || !d_merit_ref || !d_dz || !d_xu || !d_step || (rho && (!rho->rho || !rho->drho || !rho->done)))
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    { const int rc = check_steps(h, fn, step_sizes, num_steps); if (rc != MPCG_OK) return rc; }
    if (control_size == 0 || control_size > h->n) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": control_size must be 1..state_size");
    if (rho) {
        if (!std::isfinite(rho->factor) || !std::isfinite(rho->rho_min) || !std::isfinite(rho->rho_max) || !std::isfinite(rho->rho_reset))
            return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": rho_factor, rho_min, rho_max and rho_reset must be finite");
        if (!(rho->factor > T(1)) || !(rho->rho_min > T(0)) || rho->rho_max < rho->rho_min)
            return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": needs rho_factor > 1, rho_min > 0 and rho_max >= rho_min");
    }
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    WithRho ra{};
    if (rho) ra = *rho;
    Plain& a = ra;
    a.merit = d_merit; a.merit_ref = d_merit_ref; a.dz = d_dz; a.xu = d_xu; a.step = d_step; a.A = (int)num_steps;
    a.len = (size_t)(h->n + control_size) * h->N - control_size;
    for (uint32_t i = 0; i < (uint32_t)MERIT_MAX_STEPS; ++i) a.alpha[i] = i < num_steps ? step_sizes[i] : T(0);
    if (rho) hipLaunchKernelGGL(line_search_step_kernel<WithRho>, dim3(batch), dim3(256), 0, static_cast<hipStream_t>(stream), ra);
    else hipLaunchKernelGGL(line_search_step_kernel<Plain>, dim3(batch), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

template <typename T>
static int line_search_step_rho_impl(mpcg_handle* h, const char* fn, uint32_t control_size, const T* d_merit, const T* step_sizes, uint32_t num_steps,
                                     T* d_merit_ref, const T* d_dz, T* d_xu, int32_t* d_step, T* d_rho, T* d_drho, uint8_t* d_done,
                                     T rho_factor, T rho_min, T rho_max, T rho_reset, uint32_t batch, void* stream) {
    static_assert(STEP_FROZEN == MPCG_STEP_FROZEN, "the frozen code of the header");
    StepRhoArgsT<T> r{};
    r.rho = d_rho; r.drho = d_drho; r.done = d_done; r.factor = rho_factor; r.rho_min = rho_min; r.rho_max = rho_max; r.rho_reset = rho_reset;
    return line_search_step_impl<T>(h, fn, control_size, d_merit, step_sizes, num_steps, d_merit_ref, d_dz, d_xu, d_step, &r, batch, stream);
}
}  // extern "C++"

int mpcg_compute_merit(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, float timestep, const float* d_eePos_traj, const float* d_xs,
                       const float* d_xu, const float* d_dz, const float* step_sizes, uint32_t num_steps, float mu, float qd_cost, float r_cost,
                       float* d_merit, uint32_t batch, void* stream) {
    return compute_merit_impl<float>(h, "mpcg_compute_merit", plant, control_size, timestep, d_eePos_traj, d_xs, d_xu, d_dz, step_sizes, num_steps, mu, qd_cost, r_cost,
                                     d_merit, batch, stream);
}

int mpcg_compute_merit_f64(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, double timestep, const double* d_eePos_traj, const double* d_xs,
                           const double* d_xu, const double* d_dz, const double* step_sizes, uint32_t num_steps, double mu, double qd_cost, double r_cost,
                           double* d_merit, uint32_t batch, void* stream) {
    return compute_merit_impl<double>(h, "mpcg_compute_merit_f64", plant, control_size, timestep, d_eePos_traj, d_xs, d_xu, d_dz, step_sizes, num_steps, mu, qd_cost,
                                      r_cost, d_merit, batch, stream);
}

int mpcg_compute_merit_xuref(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, float timestep, const float* d_eePos_traj, const float* d_xs,
                             const float* d_xu, const float* d_dz, const float* step_sizes, uint32_t num_steps, float mu, float qd_cost, float r_cost,
                             const mpcg_xuref* ref, float* d_merit, uint32_t batch, void* stream) {
    return compute_merit_impl<float>(h, "mpcg_compute_merit_xuref", plant, control_size, timestep, d_eePos_traj, d_xs, d_xu, d_dz, step_sizes, num_steps, mu, qd_cost,
                                     r_cost, d_merit, batch, stream, true, ref);
}

int mpcg_compute_merit_xuref_f64(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, double timestep, const double* d_eePos_traj, const double* d_xs,
                                 const double* d_xu, const double* d_dz, const double* step_sizes, uint32_t num_steps, double mu, double qd_cost, double r_cost,
                                 const mpcg_xuref* ref, double* d_merit, uint32_t batch, void* stream) {
    return compute_merit_impl<double>(h, "mpcg_compute_merit_xuref_f64", plant, control_size, timestep, d_eePos_traj, d_xs, d_xu, d_dz, step_sizes, num_steps, mu,
                                      qd_cost, r_cost, d_merit, batch, stream, true, ref);
}

int mpcg_line_search_step(mpcg_handle* h, uint32_t control_size, const float* d_merit, const float* step_sizes, uint32_t num_steps,
                          float* d_merit_ref, const float* d_dz, float* d_xu, int32_t* d_step, uint32_t batch, void* stream) {
    return line_search_step_impl<float>(h, "mpcg_line_search_step", control_size, d_merit, step_sizes, num_steps, d_merit_ref, d_dz, d_xu, d_step, nullptr, batch, stream);
}

int mpcg_line_search_step_f64(mpcg_handle* h, uint32_t control_size, const double* d_merit, const double* step_sizes, uint32_t num_steps,
                              double* d_merit_ref, const double* d_dz, double* d_xu, int32_t* d_step, uint32_t batch, void* stream) {
    return line_search_step_impl<double>(h, "mpcg_line_search_step_f64", control_size, d_merit, step_sizes, num_steps, d_merit_ref, d_dz, d_xu, d_step, nullptr, batch, stream);
}

int mpcg_line_search_step_rho(mpcg_handle* h, uint32_t control_size, const float* d_merit, const float* step_sizes, uint32_t num_steps,
                              float* d_merit_ref, const float* d_dz, float* d_xu, int32_t* d_step, float* d_rho, float* d_drho, uint8_t* d_done,
                              float rho_factor, float rho_min, float rho_max, float rho_reset, uint32_t batch, void* stream) {
    return line_search_step_rho_impl<float>(h, "mpcg_line_search_step_rho", control_size, d_merit, step_sizes, num_steps, d_merit_ref, d_dz, d_xu, d_step, d_rho, d_drho,
                                            d_done, rho_factor, rho_min, rho_max, rho_reset, batch, stream);
}

int mpcg_line_search_step_rho_f64(mpcg_handle* h, uint32_t control_size, const double* d_merit, const double* step_sizes, uint32_t num_steps,
                                  double* d_merit_ref, const double* d_dz, double* d_xu, int32_t* d_step, double* d_rho, double* d_drho, uint8_t* d_done,
                                  double rho_factor, double rho_min, double rho_max, double rho_reset, uint32_t batch, void* stream) {
    return line_search_step_rho_impl<double>(h, "mpcg_line_search_step_rho_f64", control_size, d_merit, step_sizes, num_steps, d_merit_ref, d_dz, d_xu, d_step, d_rho,
                                             d_drho, d_done, rho_factor, rho_min, rho_max, rho_reset, batch, stream);
}

// ---- plant simulation and horizon shift: the step between two SQP solves (sim_plant.hip.h) ----
// mpcg_simulate (T = float) and mpcg_simulate_f64 (T = double), mpcg_advance_horizon and mpcg_advance_horizon_f64: one host path each (fn: the entry point's name);
// their _clk entries (per-trajectory clocks in device arrays) likewise, behind them
extern "C++" {
template <typename T>
static int simulate_impl(mpcg_handle* h, const char* fn, const mpcg_plant* plant, uint32_t control_size, T* d_xs, const T* d_xu, double timestep,
                         double time_offset_us, double sim_time_us, T sim_step, T* d_eePos, uint32_t batch, void* stream) {
    static_assert(SIM_MAX_SUBSTEPS == MPCG_SIM_MAX_SUBSTEPS, "the cap of the header");
    if (!h || !plant) return MPCG_ERR_INVALID;
    if (!d_xs || !d_xu) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    { const int rc = check_plant(h, fn, plant, control_size, true); if (rc != MPCG_OK) return rc; }
    if (!std::isfinite(timestep) || !std::isfinite(time_offset_us) || !std::isfinite(sim_time_us) || !std::isfinite(sim_step))
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": timestep, time_offset_us, sim_time_us and sim_step must be finite");
    if (!(sim_step > T(0)) || !(timestep > 0.0) || time_offset_us < 0.0 || sim_time_us < 0.0)
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": needs sim_step > 0, timestep > 0, time_offset_us >= 0 and sim_time_us >= 0");
    // the schedule of simple_simulate (include/common/integrator.cuh:301-322), in double
    const double ss = (double)sim_step, toff = time_offset_us * 1e-6, sim = sim_time_us * 1e-6;
    const double full = sim / ss;
    if (!(full < (double)SIM_MAX_SUBSTEPS + 1.0)) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": more than 65536 substeps (MPCG_SIM_MAX_SUBSTEPS) in one call");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    SimArgsT<T> a;
    a.plant = plant->d; a.xs = d_xs; a.xu = d_xu; a.eePos = d_eePos;
    a.N = (int)h->N; a.batch = (int)batch;
    a.S = (unsigned)full; a.ss = ss; a.toff = toff; a.timestep = timestep;
    a.rem = (double)(T)fmod(sim, ss);                        // (the reference's T: a float remainder is rounded to float, a double one is fmod's value)
    const dim3 grid((batch + KKT_ITEMS - 1) / KKT_ITEMS);
    const bool semi = h->sim_integrator == 1;      // "sim_integrator": the substep q' = q + dt qd' (0, the default: the reference's plant, explicit Euler)
    // a plant whose limits carry MPCG_LIMITS_SIM_SATURATE: the instantiation that clamps the controls it applies; any other plant: the kernels they were
    const bool saturate = plant->has_limits && (plant->lim.flags & MPCG_LIMITS_SIM_SATURATE);
    void (*const kernel)(SimArgsT<T>) = saturate ? (semi ? simulate_kernel<T, 1, 1> : simulate_kernel<T, 0, 1>) : (semi ? simulate_kernel<T, 1, 0> : simulate_kernel<T, 0, 0>);
    hipLaunchKernelGGL(kernel, grid, dim3(KKT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

template <typename T>
static int advance_horizon_impl(mpcg_handle* h, const char* fn, uint32_t control_size, uint32_t shift, T* d_xu, T* d_lambda, T* d_eePos_goal, const T* d_xs,
                                const T* d_eePos, const T* d_xu_traj, const T* d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride,
                                uint32_t xu_fill_lead, int32_t* d_traj_offset, int32_t* d_done, T* d_tracking_error, uint32_t batch, void* stream) {
    constexpr bool F64 = std::is_same<T, double>::value;
    const std::string who(fn), sim(F64 ? "mpcg_simulate_f64" : "mpcg_simulate");
    if (!h) return MPCG_ERR_INVALID;
    if (shift > 1) return fail(h, MPCG_ERR_INVALID, who + ": shift must be 0 or 1");
    if (!d_xu || !d_xs) return fail(h, MPCG_ERR_INVALID, who + ": null device pointer");
    if (shift && !d_eePos) return fail(h, MPCG_ERR_INVALID, who + ": shift = 1 needs d_eePos (the end-effector position " + sim + " wrote)");
    if (shift && (!d_lambda || !d_eePos_goal || !d_xu_traj || !d_eePos_traj || !d_traj_offset || !d_done || !d_tracking_error))
        return fail(h, MPCG_ERR_INVALID, who + ": null device pointer (shift = 1 needs every array)");
    if (control_size != (uint32_t)PJ || h->n != 2u * PJ) return fail(h, MPCG_ERR_UNSUPPORTED, who + ": state_size 14 / control_size 7 (IIWA-14) only");
    if (shift && (traj_steps == 0 || xu_fill_lead > h->N - 1 || (traj_batch_stride != 0 && traj_batch_stride < traj_steps)))
        return fail(h, MPCG_ERR_INVALID, who + ": needs traj_steps >= 1, xu_fill_lead <= knot_points - 1 and traj_batch_stride 0 or >= traj_steps");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, who + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    AdvanceArgsT<T> a;
    a.xu = d_xu; a.lambda = d_lambda; a.goal = d_eePos_goal; a.xs = d_xs; a.eePos = d_eePos; a.xu_traj = d_xu_traj; a.goal_traj = d_eePos_traj;
    a.traj_offset = d_traj_offset; a.done = d_done; a.tracking_error = d_tracking_error;
    a.n = h->n; a.m = control_size; a.N = h->N; a.traj_steps = traj_steps; a.traj_stride = traj_batch_stride; a.lead = xu_fill_lead; a.shift = shift;
    hipLaunchKernelGGL(advance_horizon_kernel<T>, dim3(batch), dim3(ADV_THREADS), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

// mpcg_simulate_clk (T = float) and mpcg_simulate_clk_f64 (T = double), mpcg_advance_horizon_clk and mpcg_advance_horizon_clk_f64: the two entries above with the
// clock in device arrays, one host path each.  What simulate_impl computes of the schedule on the host, the CLOCK = 1 kernels compute per trajectory.
template <typename T>
static int simulate_clk_impl(mpcg_handle* h, const char* fn, const mpcg_plant* plant, uint32_t control_size, T* d_xs, const T* d_xu, double timestep,
                             const double* d_time_offset_us, const double* d_sim_time_us, T sim_step, T* d_eePos, int32_t* d_done, uint32_t batch, void* stream) {
    static_assert(SIM_DONE_BAD_CLOCK == MPCG_DONE_BAD_CLOCK && ADV_DONE_BAD_CLOCK == MPCG_DONE_BAD_CLOCK, "the flag of the header");
    if (!h || !plant) return MPCG_ERR_INVALID;
    if (!d_xs || !d_xu || !d_time_offset_us || !d_sim_time_us) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    { const int rc = check_plant(h, fn, plant, control_size, true); if (rc != MPCG_OK) return rc; }
    if (!std::isfinite(timestep) || !std::isfinite(sim_step)) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": timestep and sim_step must be finite");
    if (!(sim_step > T(0)) || !(timestep > 0.0)) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": needs sim_step > 0 and timestep > 0");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    SimClkArgsT<T> a;
    a.plant = plant->d; a.xs = d_xs; a.xu = d_xu; a.eePos = d_eePos;
    a.N = (int)h->N; a.batch = (int)batch;
    a.S = 0; a.ss = (double)sim_step; a.toff = 0.0; a.timestep = timestep; a.rem = 0.0;      // (S, toff, rem: per trajectory, on the device)
    a.toff_us = d_time_offset_us; a.sim_us = d_sim_time_us; a.done = d_done;
    const dim3 grid((batch + KKT_ITEMS - 1) / KKT_ITEMS);
    const bool semi = h->sim_integrator == 1;
    const bool saturate = plant->has_limits && (plant->lim.flags & MPCG_LIMITS_SIM_SATURATE);
    void (*const kernel)(SimClkArgsT<T>) = saturate ? (semi ? simulate_kernel<T, 1, 1, 1> : simulate_kernel<T, 0, 1, 1>) : (semi ? simulate_kernel<T, 1, 0, 1> : simulate_kernel<T, 0, 0, 1>);
    hipLaunchKernelGGL(kernel, grid, dim3(KKT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

template <typename T>
static int advance_horizon_clk_impl(mpcg_handle* h, const char* fn, uint32_t control_size, T* d_xu, T* d_lambda, T* d_eePos_goal, const T* d_xs, const T* d_eePos,
                                    const T* d_xu_traj, const T* d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride, uint32_t xu_fill_lead,
                                    int32_t* d_traj_offset, int32_t* d_done, T* d_tracking_error, double timestep, double shift_threshold_s,
                                    const double* d_sim_time_us, double* d_prev_sim_us, double* d_since_s, int32_t* d_shifted, int32_t* d_did_shift, uint32_t batch,
                                    void* stream) {
    const std::string who(fn);
    if (!h) return MPCG_ERR_INVALID;
    if (!d_xu || !d_xs || !d_eePos || !d_lambda || !d_eePos_goal || !d_xu_traj || !d_eePos_traj || !d_traj_offset || !d_done || !d_tracking_error)
        return fail(h, MPCG_ERR_INVALID, who + ": null device pointer (any trajectory may shift: every array of shift = 1 is needed)");
    if (!d_sim_time_us || !d_prev_sim_us || !d_since_s || !d_shifted) return fail(h, MPCG_ERR_INVALID, who + ": null time or clock array");
    if (control_size != (uint32_t)PJ || h->n != 2u * PJ) return fail(h, MPCG_ERR_UNSUPPORTED, who + ": state_size 14 / control_size 7 (IIWA-14) only");
    if (traj_steps == 0 || xu_fill_lead > h->N - 1 || (traj_batch_stride != 0 && traj_batch_stride < traj_steps))
        return fail(h, MPCG_ERR_INVALID, who + ": needs traj_steps >= 1, xu_fill_lead <= knot_points - 1 and traj_batch_stride 0 or >= traj_steps");
    if (!std::isfinite(timestep) || !(timestep > 0.0) || !std::isfinite(shift_threshold_s) || shift_threshold_s < 0.0)
        return fail(h, MPCG_ERR_INVALID, who + ": needs a finite timestep > 0 and a finite shift_threshold_s >= 0");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, who + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    AdvanceClkArgsT<T> a;
    a.xu = d_xu; a.lambda = d_lambda; a.goal = d_eePos_goal; a.xs = d_xs; a.eePos = d_eePos; a.xu_traj = d_xu_traj; a.goal_traj = d_eePos_traj;
    a.traj_offset = d_traj_offset; a.done = d_done; a.tracking_error = d_tracking_error;
    a.n = h->n; a.m = control_size; a.N = h->N; a.traj_steps = traj_steps; a.traj_stride = traj_batch_stride; a.lead = xu_fill_lead; a.shift = 1;
    a.timestep = timestep; a.threshold = shift_threshold_s;
    a.sim_us = d_sim_time_us; a.prev_us = d_prev_sim_us; a.since = d_since_s; a.shifted = d_shifted; a.did_shift = d_did_shift;
    hipLaunchKernelGGL(advance_horizon_clk_kernel<T>, dim3(batch), dim3(ADV_THREADS), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}
}  // extern "C++"

int mpcg_simulate(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, float* d_xs, const float* d_xu, double timestep, double time_offset_us,
                  double sim_time_us, float sim_step, float* d_eePos, uint32_t batch, void* stream) {
    return simulate_impl<float>(h, "mpcg_simulate", plant, control_size, d_xs, d_xu, timestep, time_offset_us, sim_time_us, sim_step, d_eePos, batch, stream);
}

int mpcg_simulate_f64(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, double* d_xs, const double* d_xu, double timestep, double time_offset_us,
                      double sim_time_us, double sim_step, double* d_eePos, uint32_t batch, void* stream) {
    return simulate_impl<double>(h, "mpcg_simulate_f64", plant, control_size, d_xs, d_xu, timestep, time_offset_us, sim_time_us, sim_step, d_eePos, batch, stream);
}

// ---- batched inverse dynamics (invdyn_plant.hip.h): mpcg_inverse_dynamics (T = float) and mpcg_inverse_dynamics_f64 (T = double), one host path ----
extern "C++" {
template <typename T>
static int inverse_dynamics_impl(mpcg_handle* h, const char* fn, const mpcg_plant* plant, const T* d_q, const T* d_qd, const T* d_qdd, T* d_tau, uint32_t count, void* stream) {
    if (!h || !plant) return MPCG_ERR_INVALID;
    if (!d_q || !d_tau) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    if (h->n != 2u * PJ) return fail(h, MPCG_ERR_UNSUPPORTED, std::string(fn) + ": state_size 14 (IIWA-14) only");      // (no control size: the entry's own words)
    { const int rc = check_plant(h, fn, plant, PJ, true); if (rc != MPCG_OK) return rc; }
    if (count == 0) return MPCG_OK;
    if ((uint64_t)count > (uint64_t)h->max_batch * h->N) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": count exceeds max_batch x knot_points");
    HIP_TRY(h, hipSetDevice(h->device));
    InvDynArgsT<T> a;
    a.plant = plant->d; a.q = d_q; a.qd = d_qd; a.qdd = d_qdd; a.tau = d_tau; a.count = count;
    hipLaunchKernelGGL(inverse_dynamics_kernel<T>, dim3((count + KKT_ITEMS - 1) / KKT_ITEMS), dim3(KKT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}
}  // extern "C++"

int mpcg_inverse_dynamics(mpcg_handle* h, const mpcg_plant* plant, const float* d_q, const float* d_qd, const float* d_qdd, float* d_tau, uint32_t count, void* stream) {
    return inverse_dynamics_impl<float>(h, "mpcg_inverse_dynamics", plant, d_q, d_qd, d_qdd, d_tau, count, stream);
}

int mpcg_inverse_dynamics_f64(mpcg_handle* h, const mpcg_plant* plant, const double* d_q, const double* d_qd, const double* d_qdd, double* d_tau, uint32_t count,
                              void* stream) {
    return inverse_dynamics_impl<double>(h, "mpcg_inverse_dynamics_f64", plant, d_q, d_qd, d_qdd, d_tau, count, stream);
}

int mpcg_advance_horizon(mpcg_handle* h, uint32_t control_size, uint32_t shift, float* d_xu, float* d_lambda, float* d_eePos_goal, const float* d_xs,
                         const float* d_eePos, const float* d_xu_traj, const float* d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride,
                         uint32_t xu_fill_lead, int32_t* d_traj_offset, int32_t* d_done, float* d_tracking_error, uint32_t batch, void* stream) {
    return advance_horizon_impl<float>(h, "mpcg_advance_horizon", control_size, shift, d_xu, d_lambda, d_eePos_goal, d_xs, d_eePos, d_xu_traj, d_eePos_traj, traj_steps,
                                       traj_batch_stride, xu_fill_lead, d_traj_offset, d_done, d_tracking_error, batch, stream);
}

int mpcg_advance_horizon_f64(mpcg_handle* h, uint32_t control_size, uint32_t shift, double* d_xu, double* d_lambda, double* d_eePos_goal, const double* d_xs,
                             const double* d_eePos, const double* d_xu_traj, const double* d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride,
                             uint32_t xu_fill_lead, int32_t* d_traj_offset, int32_t* d_done, double* d_tracking_error, uint32_t batch, void* stream) {
    return advance_horizon_impl<double>(h, "mpcg_advance_horizon_f64", control_size, shift, d_xu, d_lambda, d_eePos_goal, d_xs, d_eePos, d_xu_traj, d_eePos_traj,
                                        traj_steps, traj_batch_stride, xu_fill_lead, d_traj_offset, d_done, d_tracking_error, batch, stream);
}

int mpcg_simulate_clk(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, float* d_xs, const float* d_xu, double timestep, const double* d_time_offset_us,
                      const double* d_sim_time_us, float sim_step, float* d_eePos, int32_t* d_done, uint32_t batch, void* stream) {
    return simulate_clk_impl<float>(h, "mpcg_simulate_clk", plant, control_size, d_xs, d_xu, timestep, d_time_offset_us, d_sim_time_us, sim_step, d_eePos, d_done, batch,
                                    stream);
}

int mpcg_simulate_clk_f64(mpcg_handle* h, const mpcg_plant* plant, uint32_t control_size, double* d_xs, const double* d_xu, double timestep,
                          const double* d_time_offset_us, const double* d_sim_time_us, double sim_step, double* d_eePos, int32_t* d_done, uint32_t batch, void* stream) {
    return simulate_clk_impl<double>(h, "mpcg_simulate_clk_f64", plant, control_size, d_xs, d_xu, timestep, d_time_offset_us, d_sim_time_us, sim_step, d_eePos, d_done,
                                     batch, stream);
}

int mpcg_advance_horizon_clk(mpcg_handle* h, uint32_t control_size, float* d_xu, float* d_lambda, float* d_eePos_goal, const float* d_xs, const float* d_eePos,
                             const float* d_xu_traj, const float* d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride, uint32_t xu_fill_lead,
                             int32_t* d_traj_offset, int32_t* d_done, float* d_tracking_error, double timestep, double shift_threshold_s, const double* d_sim_time_us,
                             double* d_prev_sim_us, double* d_since_s, int32_t* d_shifted, int32_t* d_did_shift, uint32_t batch, void* stream) {
    return advance_horizon_clk_impl<float>(h, "mpcg_advance_horizon_clk", control_size, d_xu, d_lambda, d_eePos_goal, d_xs, d_eePos, d_xu_traj, d_eePos_traj, traj_steps,
                                           traj_batch_stride, xu_fill_lead, d_traj_offset, d_done, d_tracking_error, timestep, shift_threshold_s, d_sim_time_us,
                                           d_prev_sim_us, d_since_s, d_shifted, d_did_shift, batch, stream);
}

int mpcg_advance_horizon_clk_f64(mpcg_handle* h, uint32_t control_size, double* d_xu, double* d_lambda, double* d_eePos_goal, const double* d_xs, const double* d_eePos,
                                 const double* d_xu_traj, const double* d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride, uint32_t xu_fill_lead,
                                 int32_t* d_traj_offset, int32_t* d_done, double* d_tracking_error, double timestep, double shift_threshold_s,
                                 const double* d_sim_time_us, double* d_prev_sim_us, double* d_since_s, int32_t* d_shifted, int32_t* d_did_shift, uint32_t batch,
                                 void* stream) {
    return advance_horizon_clk_impl<double>(h, "mpcg_advance_horizon_clk_f64", control_size, d_xu, d_lambda, d_eePos_goal, d_xs, d_eePos, d_xu_traj, d_eePos_traj,
                                            traj_steps, traj_batch_stride, xu_fill_lead, d_traj_offset, d_done, d_tracking_error, timestep, shift_threshold_s,
                                            d_sim_time_us, d_prev_sim_us, d_since_s, d_shifted, d_did_shift, batch, stream);
}

}  // extern "C"
