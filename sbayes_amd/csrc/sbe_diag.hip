// sbe_diag.hip -- convergence diagnostics per column on the device (include/sbe_diag.h): the float64 store of M chains,
// its fill kernel, and one workgroup per column computing mean, sd, ESS (Geyer's initial positive and initial monotone
// sequence), R-hat and the Monte-Carlo standard error of the mean.  The numerical contract is tests/_diag_oracle.py;
// DESIGN.md section 16 has the layout, the launch rule and the limits.  The store, the plan of a compute call and the
// column kernel live in sbe_diag_column.hip.h, which sbe_summary.hip shares.
#include "sbe_diag_column.hip.h"

struct sbe_diag : sbe_unit_handle, diag_store {   // (sbe_unit.hip.h; ev: around the column kernel of the last compute call)
    double* d_out = nullptr;            // [5][P]
    size_t out_bytes = 0;
    int32_t* d_lags = nullptr;          // [P]
    size_t lags_bytes = 0;
    uint8_t* d_flag = nullptr;          // [P]
    size_t flag_bytes = 0;
    int64_t launch_columns = 0;         // 0: the default
    int last_M = 0, last_path = 0;
    int64_t last_n = 0, last_launches = 0;
    std::vector<void*> buffers() const { return {d_x, d_stage, d_out, d_lags, d_flag, d_off, d_scratch}; }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr char kReset[] = "sbe_diag_reset";

}  // namespace

extern "C" {

int sbe_diag_abi_version(void) { return SBE_DIAG_ABI_VERSION; }

const char* sbe_diag_last_error(const sbe_diag* h) { return unit_last_error(h); }

int64_t sbe_diag_lds_max_draws(void) { return kLdsMaxDraws; }

int sbe_diag_create(sbe_diag** out, int device) { return unit_create_on_device(out, device, "sbe_diag_create"); }

int sbe_diag_destroy(sbe_diag* h) { return unit_destroy(h, kNullHandle); }

int sbe_diag_last_kernel_ms(const sbe_diag* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int sbe_diag_set_launch_columns(sbe_diag* h, int64_t columns) {
    CHECK_HANDLE(h, kNullHandle);
    if (columns < 0 || columns > kMaxGridBlocks)
        return fail(h, SBE_ERR_ARG, "columns=%lld out of range [0, %lld] (0: the default)", (long long)columns, (long long)kMaxGridBlocks);
    h->launch_columns = columns;
    return SBE_OK;
}

int sbe_diag_reset(sbe_diag* h, int n_chains, int64_t n_columns, int64_t capacity_rows) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = diag_store_reset(h, n_chains, n_columns, capacity_rows);
    if (!rc) rc = unit_ensure(h, h->d_out, h->out_bytes, (size_t)n_columns * 5 * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_lags, h->lags_bytes, (size_t)n_columns * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_flag, h->flag_bytes, (size_t)n_columns);
    if (rc) return rc;
    diag_store_shaped(h, n_chains, n_columns, capacity_rows);
    return SBE_OK;
}

int sbe_diag_rows(const sbe_diag* h, int chain, int64_t* n_rows_out) {
    CHECK_HANDLE(h, kNullHandle);
    return h->chains.get(h, kDiagLane, chain, n_rows_out);
}

int sbe_diag_append_rows(sbe_diag* h, int chain, const double* rows, int64_t n_rows) {
    CHECK_HANDLE(h, kNullHandle);
    return diag_store_append(h, kReset, chain, rows, n_rows);
}

int sbe_diag_compute(sbe_diag* h, const int64_t* burn_rows, int split, int64_t max_lag, double* mean_out, double* sd_out,
                     double* ess_out, double* rhat_out, double* mcse_mean_out, int32_t* n_lags_out, uint8_t* flag_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->chains.check_shaped(h, kReset)) return rc;
    if (!burn_rows) return fail(h, SBE_ERR_ARG, "null pointer argument: burn_rows");
    if (!mean_out || !sd_out || !ess_out || !rhat_out || !mcse_mean_out || !n_lags_out || !flag_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    int M = 0;
    int64_t n = 0;
    std::vector<int64_t> off;
    if (const int rc = diag_plan(h, kReset, burn_rows, split, max_lag, &M, &n, &off)) return rc;
    const int64_t per_launch = diag_per_launch(h->launch_columns, M, n, h->P);
    HIPCHK(h, hipSetDevice(h->device));
    if (const int rc = diag_prepare_launch(h, M, n, per_launch)) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_off, off.data(), (size_t)M * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    int64_t launches = 0;
    int rc = unit_timed(h, [&] {
        return diag_launch_columns(h, h->d_x, h->d_off, h->chains.cap, M, n, max_lag, h->d_out, h->d_lags, h->d_flag, h->P, h->P, per_launch, &launches);
    });
    const size_t P = (size_t)h->P;
    if (!rc) rc = unit_copy_back(h, (const double*)h->d_out, P, {mean_out, sd_out, ess_out, rhat_out, mcse_mean_out});
    if (!rc) rc = unit_copy_back(h, (const int32_t*)h->d_lags, P, {n_lags_out});
    if (!rc) rc = unit_copy_back(h, (const uint8_t*)h->d_flag, P, {flag_out});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->last_M = M;
    h->last_n = n;
    h->last_path = diag_staged(M, n) ? SBE_DIAG_PATH_LDS : SBE_DIAG_PATH_GLOBAL;
    h->last_launches = launches;
    return SBE_OK;
}

int sbe_diag_last_shape(const sbe_diag* h, int* chains_out, int64_t* draws_out, int* path_out, int64_t* launches_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!chains_out || !draws_out || !path_out || !launches_out) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    *chains_out = h->last_M;
    *draws_out = h->last_n;
    *path_out = h->last_path;
    *launches_out = h->last_launches;
    return SBE_OK;
}

}  // extern "C"
