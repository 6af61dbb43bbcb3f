// mpcg_riccati.hip — C ABI (include/mpcg_riccati.h) of the Riccati feedback gains: ONE host path, riccati_impl<IO>, for the float and the
// double entry, and one kernel body (riccati.hip.h) in two builds per storage type: (14, 7) at compile time, run-time dimensions for every
// other shape.  Pure stream work: no handle buffer, no option, nothing latched on the handle.
#include "mpcg_handle.hpp"
#include "../../include/mpcg_riccati.h"
#include <cmath>
#include "riccati.hip.h"

using namespace mpcg;

static constexpr size_t kRicLdsMax = 160 * 1024;       // LDS of one CU: what one wavefront's operands may occupy

template <typename IO>
static int riccati_impl(mpcg_handle* h, const char* fn, uint32_t control_size, const IO* d_G, const IO* d_C, IO rho, const IO* d_rho, IO* d_K,
                        uint32_t batch, void* stream) {
    if (!h) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null handle");
    if (!d_G || !d_C || !d_K) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    if (control_size == 0 || control_size > h->n)
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": control_size must be between 1 and state_size");
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    if (!d_rho && !(std::isfinite(rho) && rho >= IO(0)))
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": rho must be finite and >= 0 (or pass d_rho, one value per trajectory)");
    if (batch == 0 || h->N < 2) return MPCG_OK;        // no trajectory; one knot: no controls, nothing to write
    const int n = (int)h->n, m = (int)control_size;
    const size_t lds = ric::riccati_lds_doubles(n, m) * sizeof(double);
    if (lds > kRicLdsMax)
        return fail(h, MPCG_ERR_UNSUPPORTED, std::string(fn) + ": the operands of one trajectory (" + std::to_string(lds) + " bytes at state_size " + std::to_string(n) +
                    ", control_size " + std::to_string(m) + ") exceed the LDS limit of 160 KiB (8 (LD^2 + 2 LD (n + m) + LM (m + 2 n)) bytes, LD, LM = n, m rounded up to 4)");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ric::RiccatiArgsT<IO> a{d_G, d_C, d_rho, d_K, (double)rho, n, m, (int)h->N};
    if (n == 14 && m == 7) {
        hipLaunchKernelGGL((ric::riccati_gains_kernel<IO, 14, 7>), dim3(batch), dim3(64), lds, st, a);
    } else {
        // (as the LDS producers: beyond 48 KiB of dynamic LDS the kernel's limit is raised first)
        if (lds > 48 * 1024)
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(ric::riccati_gains_kernel<IO, 0, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((ric::riccati_gains_kernel<IO, 0, 0>), dim3(batch), dim3(64), lds, st, a);
    }
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

extern "C" {

int mpcg_riccati_gains(mpcg_handle* h, uint32_t control_size, const float* d_G_dense, const float* d_C_dense, float rho, const float* d_rho,
                       float* d_K, uint32_t batch, void* stream) {
    return riccati_impl<float>(h, "mpcg_riccati_gains", control_size, d_G_dense, d_C_dense, rho, d_rho, d_K, batch, stream);
}

int mpcg_riccati_gains_f64(mpcg_handle* h, uint32_t control_size, const double* d_G_dense, const double* d_C_dense, double rho, const double* d_rho,
                           double* d_K, uint32_t batch, void* stream) {
    return riccati_impl<double>(h, "mpcg_riccati_gains_f64", control_size, d_G_dense, d_C_dense, rho, d_rho, d_K, batch, stream);
}

}  // extern "C"
