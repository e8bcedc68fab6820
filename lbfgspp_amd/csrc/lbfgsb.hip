// lbfgspp_amd/csrc/lbfgsb.hip -- L-BFGS-B device operators, core: the per-context state's allocation and release, the helpers every phase
// uses (lbfgsb_state.hpp has the map of the mechanisms), lbfgsx_b_reserve and the process-wide counters.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#define LBFGSB_TU "lbfgsb"
#include "lbfgsb_state.hpp"

namespace lbfgsx {

// instrumentation, process-wide: {subspace minimisations that ran on compact vectors, times they went back to their rows
// before the minimisation assigned its result}
static std::atomic<int64_t> g_cv_starts{0}, g_cv_backs{0}, g_wtdc_runs{0}, g_stash_hits{0};
void count_cv_start() { g_cv_starts.fetch_add(1, std::memory_order_relaxed); }
void count_wtdc_run() { g_wtdc_runs.fetch_add(1, std::memory_order_relaxed); }
void count_stash_hit() { g_stash_hits.fetch_add(1, std::memory_order_relaxed); }

int cv_alloc(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    if (b->cv_buf && b->cv_cap >= c->ld)
        return LBFGSX_OK;
    if (b->cv_buf)
        (void) hipFree(b->cv_buf);
    b->cv_buf = nullptr;
    b->cv_cap = c->ld;
    if (hipMalloc(&b->cv_buf, size_t(b->cv_cap) * (8 * c->esz + 1) + 64) != hipSuccess)
    {
        (void) hipGetLastError();
        b->cv_buf = nullptr;
        b->cv_cap = 0;
        return LBFGSX_E_HIP;  // the caller simply keeps the vectors at their rows
    }
    return LBFGSX_OK;
}
// put the compact vectors back at their rows; assign: only what subvec_assign(drt, fv_set, vecy) needs (+ the state bytes)
int cv_back(lbfgsx_ctx* c, bool assign)
{
    lbfgsb_state* b = c->bstate;
    if (!b->cv_live)
        return LBFGSX_OK;
    b->cv_live = false;
    if (!assign)
    {
        b->cv_backs++;
        g_cv_backs.fetch_add(1, std::memory_order_relaxed);
    }
    const int64_t npos = b->wf_n;
    const int grid = std::max(1, std::min(c->grid_for(2 * npos), 1024));
    // byte model: state byte, row number and y of every position read; written by row (sectors): the state byte and drt, or the
    // five compact vectors
    lbfgsx::model_add(double(npos) * (1 + 4 + double(c->esz) * (assign ? 1 : 5)) + (assign ? 0.0 : lbfgsx::model_gather(npos, c->n, 1)) +
                      (assign ? 1 : 5) * lbfgsx::model_gather(npos, c->n, int(c->esz)));
    DISPATCH_T(c, {
        if (assign)
            LBFGSX_LAUNCH((k_cv_back<T, 1>), dim3(grid), dim3(kBlock), 0, c->stream, bvecs<T>(c), bvecs_cv<T>(c), b->wf_idx, npos);
        else
            LBFGSX_LAUNCH((k_cv_back<T, 0>), dim3(grid), dim3(kBlock), 0, c->stream, bvecs<T>(c), bvecs_cv<T>(c), b->wf_idx, npos);
    });
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}
int need_bounded(lbfgsx_ctx* c, bool keep_force, bool keep_cv, bool keep_stash, bool keep_fin)
{
    if (!c->bstate)
    {
        set_error("this context was not created with LBFGSX_FLAG_BOUNDED");
        return LBFGSX_E_LOGIC;
    }
    c->st_valid = false;  // any entry of the bounded path may change what a trial evaluated ahead was computed from
    if (!keep_fin)  // what lbfgsx_b_cauchy_finish left for the two entries that follow it (sub_begin, W_A'(A'd))
    {
        c->bstate->drt_ready = false;
        c->bstate->na_n = -1;
    }
    if (!keep_stash)
        for (int q = 0; q < 3; q++)
            c->bstate->stash_valid[q] = c->bstate->stash_armed[q] = false;
    lbfgsx::poll_disarm(c);  // an entry starts with no completion word armed (an error path may have left one)
    if (c->bstate->cv_live && !keep_cv)
    {
        lbfgsx::DeviceGuard dev_guard_(c->device);
        const int rc = cv_back(c, false);
        if (rc)
            return rc;
    }
    if (c->bstate->force_pending && !keep_force)
    {
        c->bstate->force_pending = false;
        return run_force_bounds(c);
    }
    return LBFGSX_OK;
}

int upload_phys(lbfgsx_ctx* c)
{
    if (c->bstate->phys_seen == c->phys_version)  // the map changes once per accepted correction, the operators
        return LBFGSX_OK;                         // that read it run a dozen times per iteration
    c->bstate->phys_seen = c->phys_version;
    LBFGSX_HIP(lbfgsx::copy_async(c->bstate->phys_dev, c->phys.data(), sizeof(int) * size_t(c->m), hipMemcpyHostToDevice, c->stream));
    return LBFGSX_OK;
}

int fetch_doubles(lbfgsx_ctx* c, int k, double* out)
{
    if (c->bstate->dout_host)
    {
        // dout is host-mapped: the kernel's stores are visible once the stream has drained (no copy kernel) -- or, after a
        // poll_arm, once the kernel's completion word has arrived
        LBFGSX_HIP(lbfgsx::poll_wait(c));
        const volatile double* h = c->bstate->dout_host;
        for (int i = 0; i < k; i++)
            out[i] = h[i];
        return LBFGSX_OK;
    }
    LBFGSX_HIP(lbfgsx::copy_async(c->hout, c->bstate->dout, sizeof(double) * size_t(k), hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    std::memcpy(out, c->hout, sizeof(double) * size_t(k));
    return LBFGSX_OK;
}

template <class T>
int fetch_T(lbfgsx_ctx* c, int idx, int k, double* out)
{
    if (idx == c->sl.out(0) && c->outmap_dev)
    {
        LBFGSX_HIP(lbfgsx::poll_wait(c));
        const volatile T* h = static_cast<const volatile T*>(c->outmap_host);
        for (int i = 0; i < k; i++)
            out[i] = double(h[i]);
        return LBFGSX_OK;
    }
    LBFGSX_HIP(lbfgsx::copy_async(c->hout, P<T>(c->sc) + idx, sizeof(T) * size_t(k), hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    const T* h = static_cast<const T*>(c->hout);
    for (int i = 0; i < k; i++)
        out[i] = double(h[i]);
    return LBFGSX_OK;
}

template int fetch_T<float>(lbfgsx_ctx*, int, int, double*);
template int fetch_T<double>(lbfgsx_ctx*, int, int, double*);

int bounded_alloc(lbfgsx_ctx* c)
{
    lbfgsb_state* b = new lbfgsb_state();
    c->bstate = b;
    const size_t vbytes = size_t(c->ld) * c->esz;
    void** vecs[] = {&b->brk, &b->dvec, &b->cF, &b->y, &b->yfb, &b->lam, &b->mu, &b->rhs, &b->keys_in, &b->keys_out};
    for (void** v : vecs)
        LBFGSX_HIP(hipMalloc(v, vbytes));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->st), size_t(c->ld)));
    LBFGSX_HIP(hipMemset(b->st, 0, size_t(c->ld)));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->vals_in), sizeof(int) * size_t(c->ld)));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->vals_out), sizeof(int) * size_t(c->ld)));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->phys_dev), sizeof(int) * size_t(c->m + 1)));
    if (c->outmap_dev)
    {
        LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->dout_host), sizeof(double) * lbfgsb_state::kDout, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(b->dout_host, 0, sizeof(double) * lbfgsb_state::kDout);
        LBFGSX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->dout), b->dout_host, 0));
    }
    else
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->dout), sizeof(double) * lbfgsb_state::kDout));
    LBFGSX_HIP(hipMalloc(&b->coef_dev, sizeof(double) * 80));
    b->lu_cap = unsigned(std::min<int64_t>(c->n, int64_t(1) << 20));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->lu_list), sizeof(int) * 2 * size_t(b->lu_cap)));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->lu_cnt), sizeof(unsigned)));
    LBFGSX_HIP(hipMemset(b->lu_cnt, 0, sizeof(unsigned)));
    if (const char* e = getenv("LBFGSX_SWEEP_SOLVE_FUSE"))
        b->sweep_fuse = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_COMPACT_FREE"))
        b->wf_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_SPLIT"))
        b->split = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_FINISH_FUSE"))
        b->fin_fuse = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_NEWACT_CAP"))  // test aid: a short list overflows
        b->na_cap = unsigned(std::max(1, std::min(1 << 20, atoi(e))));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->na_list), sizeof(int) * size_t(b->na_cap)));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->na_cnt), sizeof(unsigned)));
    LBFGSX_HIP(hipMemset(b->na_cnt, 0, sizeof(unsigned)));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->xp1), sizeof(double) * size_t(kMaxGridX) * kMaxSumsX * 2));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->xp2), sizeof(double) * size_t(kMaxGridX / kGroupX) * kMaxSumsX * 2));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->xtickets), sizeof(unsigned) * (2 + kMaxGridX / kGroupX)));
    LBFGSX_HIP(hipMemset(b->xtickets, 0, sizeof(unsigned) * (2 + kMaxGridX / kGroupX)));
    b->gtile = std::max(3, xl::gram_kpb(2 * c->m + 1));
    if (const char* e = getenv("LBFGSX_COMPACT_VEC"))
        b->cv_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_WTD_COMPACT"))
        b->wtdc_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_SELECT_INLINE"))
        b->psel_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_POST_BUILD"))
        b->pb_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_TRIAL_AHEAD"))
        b->st_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_RHS_IDENTITY"))
        b->rhs_identity = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_CHUNK_AHEAD"))
        b->gpre_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_DELTA_AHEAD"))
        b->fd_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_LIST12"))
        b->list12 = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_PSEL_SMALL"))  // 0: a short candidate list is ordered by the three launches of round 4
        b->psel_small = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_SELECT_CAP"))  // test aid: a short list overflows
        b->psel_cap = unsigned(std::max(1, std::min(1 << 24, atoi(e))));
    if (const char* e = getenv("LBFGSX_SYNC_MERGE"))
        b->stash_use = atoi(e) != 0;
    if (const char* e = getenv("LBFGSX_WTD_LIST_CAP"))  // test aid: a short list overflows
        b->wtdc_cap = unsigned(std::max(1, std::min(1 << 20, atoi(e))));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->colmax), sizeof(unsigned long long) * 2 * size_t(c->m + 1)));
    LBFGSX_HIP(hipMemset(b->colmax, 0, sizeof(unsigned long long) * 2 * size_t(c->m + 1)));
    b->colmax_ok.assign(size_t(c->m + 1), 0);
    // radix sort temporary storage
    const size_t bytes = sort_pairs_tmp_bytes(c);
    // Which kernel forms a full W_F'W_F.  The double-double VALU kernel costs ~ (2c + 1)^2 per row; the exact integer
    // kernel on the matrix cores (gram_i8.cuh, LBFGSX_GRAM=i8) is flat up to 32 columns but bound by the ~1000 VALU
    // instructions per 32 rows that cut the radix-256 digits.  Measured on MI355X (n = 1e7, ~5e6 free rows, the pass also
    // writing the compact copy of the free rows; profiles/r3_gram_dd_vs_i8.txt): 0.74 / 1.35 / 1.71 / 1.75 ms against
    // 0.73 / 1.41 / 1.48 / 1.51 ms at m = 10 / 12 / 14 / 15 -- the matrix-core kernel is the faster one from m = 14 on,
    // by 14 % of a pass that is a quarter of an iteration there.  End to end that is +1 % steady and -4 % from x0 at
    // m = 15 (its per-column maxima cost a little in every iteration, k_b_post), and a loss below; at m <= 10 the question
    // does not arise in the steady state, W_F'W_F being carried between iterations (one full pass in 32).  So the
    // double-double kernel stays the default at every m and the matrix-core kernel an option that changes no bit.
    if (const char* e = getenv("LBFGSX_GRAM"))
    {
        b->gram_i8 = (std::strcmp(e, "i8") == 0);
        if (const char* e2 = getenv("LBFGSX_GRAM_I8_MIN"))
            b->i8_min_tot = std::max(1, atoi(e2));
        b->gram_mode = (std::strcmp(e, "blocked") == 0) ? 2 : 0;
        // "dd" / "" name the default; anything else (e.g. the removed "mfma") is a typo that would silently measure the
        // default path under another name
        if (!b->gram_i8 && b->gram_mode == 0 && e[0] != 0 && std::strcmp(e, "dd") != 0)
        {
            static bool warned = false;
            if (!warned)
                fprintf(stderr, "lbfgsx: LBFGSX_GRAM=%s is not a Gram kernel (i8, blocked, dd): using the default\n", e);
            warned = true;
        }
    }
    if (const char* e = getenv("LBFGSX_GCP_CHAIN"))
        b->chain_host = std::strcmp(e, "scan") != 0;
    if (const char* e = getenv("LBFGSX_MULTIDOT"))
        b->multidot_chunked = (std::strcmp(e, "chunked") == 0);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0)
            b->num_cus = prop.multiProcessorCount;
    }
    const size_t gent = size_t(b->gtile) * 256;  // entries the Gram buffers hold
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->gram_partial), sizeof(double) * size_t(lbfgsb_state::kGramBlocks) * gent * 2));
    LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->gram_partial2), sizeof(double) * 32 * gent * 2));
    if (c->outmap_dev)
    {
        // the (hi, lo) sums land where the host reads them: a copy into pageable memory is staged and costs ~20 us a fetch
        LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->gram_dd_host), sizeof(double) * gent * 2, hipHostMallocMapped | hipHostMallocCoherent));
        LBFGSX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->gram_dd), b->gram_dd_host, 0));
        LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->stash_host), sizeof(double) * 3 * (gent * 3), hipHostMallocMapped | hipHostMallocCoherent));
        LBFGSX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->stash_dev), b->stash_host, 0));
        LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->gram_out_host), sizeof(double) * gent, hipHostMallocMapped | hipHostMallocCoherent));
        LBFGSX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->gram_out), b->gram_out_host, 0));
    }
    else
    {
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->gram_out), sizeof(double) * gent));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->gram_dd), sizeof(double) * gent * 2));
    }
    b->sort_tmp_bytes = bytes;
    LBFGSX_HIP(hipMalloc(&b->sort_tmp, bytes ? bytes : 16));
    return LBFGSX_OK;
}

void bounded_free(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    if (!b)
        return;
    void* ptrs[] = {b->brk, b->dvec, b->cF, b->y, b->yfb, b->lam, b->mu, b->rhs, b->keys_in, b->keys_out, b->st,
                    b->vals_in, b->vals_out, b->phys_dev, b->dout, b->coef_dev, b->sort_tmp, b->g_brk,
                    b->g_g, b->g_z, b->g_w, b->g_idx, b->gram_partial, b->gram_partial2, b->gram_out, b->gram_dd,
                    b->s_brk, b->s_g, b->s_z, b->s_W, b->s_P, b->s_C, b->s_chain, b->s_ts, b->s_off,
                    b->s_small, b->s_exit, b->pk, b->pv, b->pcount, b->sel_tmp};
    if (b->h_chain)
        (void) hipHostFree(b->h_chain);
    if (b->exit_map_host)
        (void) hipHostFree(b->exit_map_host);
    if (b->gout_host)
        (void) hipHostFree(b->gout_host);
    if (b->g_host)
        (void) hipHostFree(b->g_host);
    if (b->fd_host)
        (void) hipHostFree(b->fd_host);
    (void) hipFree(b->lu_list);
    (void) hipFree(b->wf_pos);
    (void) hipFree(b->wtdc_list);
    (void) hipFree(b->wtdc_cnt);
    (void) hipFree(b->psel_list);
    (void) hipFree(b->psel_cnt);
    (void) hipFree(b->psel_tmp);
    for (hipEvent_t ev : b->chain_ev)
        if (ev)
            (void) hipEventDestroy(ev);
    (void) hipFree(b->fprev);
    (void) hipFree(b->dl_enter);
    (void) hipFree(b->dl_leave);
    (void) hipFree(b->dl_cnt);
    (void) hipFree(b->wf);
    (void) hipFree(b->wf_idx);
    (void) hipFree(b->wf_cnt);
    (void) hipFree(b->wf_base);
    (void) hipFree(b->wf_tmp);
    (void) hipFree(b->lu_cnt);
    (void) hipFree(b->colmax);
    (void) hipFree(b->i8_part);
    (void) hipFree(b->i8_partv);
    (void) hipFree(b->i8_vsum);
    for (void* p : ptrs)
    {
        // dout / gram_out are device aliases of host-mapped memory when the mapped outputs are on
        if ((p == b->dout && b->dout_host) || (p == b->gram_out && b->gram_out_host) || (p == b->gram_dd && b->gram_dd_host))
            continue;
        (void) hipFree(p);
    }
    if (b->dout_host)
        (void) hipHostFree(b->dout_host);
    if (b->gram_out_host)
        (void) hipHostFree(b->gram_out_host);
    if (b->gram_dd_host)
        (void) hipHostFree(b->gram_dd_host);
    if (b->stash_host)
        (void) hipHostFree(b->stash_host);
    (void) hipFree(b->cv_buf);
    (void) hipFree(b->na_list);
    (void) hipFree(b->na_cnt);
    (void) hipFree(b->xp1);
    (void) hipFree(b->xp2);
    (void) hipFree(b->xtickets);
    delete b;
    c->bstate = nullptr;
}

RedWsX wsx(lbfgsx_ctx* c)  // after poll_arm: carries the completion word of this launch
{
    RedWsX w;
    w.p1 = c->bstate->xp1;
    w.p2 = c->bstate->xp2;
    w.tickets = c->bstate->xtickets;
    w.done = c->ws.done;
    w.seq = c->ws.seq;
    return w;
}
// keys_in / vals_in as a full radix sort (or a selection over all n keys) reads them: rebuilt from brk when the build left them
// out (k_b_post_build with the partial sort's candidates listed in the pass: lbfgsx_b_post_linesearch_build)
int ensure_keys(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    if (b->keys_valid && b->vals_iota)
        return LBFGSX_OK;
    const int grid = c->grid_for(c->n);
    DISPATCH_T(c, {
        lbfgsx::model_add(double(c->n) * (2 * sizeof(T) + (b->vals_iota ? 0 : 4)));
        LBFGSX_LAUNCH((k_keys_from_brk<T>), dim3(grid), dim3(kBlock), 0, c->stream, static_cast<const T*>(b->brk),
                      static_cast<T*>(b->keys_in), b->vals_iota ? static_cast<int*>(nullptr) : b->vals_in, c->n);
    });
    LBFGSX_HIP(hipGetLastError());
    b->keys_valid = true;
    b->vals_iota = true;
    return LBFGSX_OK;
}

// after a pass has written the compact copy afresh: usable now, and kept for the next iteration's carried first solve
void wf_rebuilt(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    b->wf_valid = true;
    b->wf_n = b->nfree_last;
    b->wf_live = true;
    b->wf_ncorr = c->ncorr;
    b->wf_epoch = b->sub_epoch;
}

// can this iteration's W'd come from the kept compact copy?  Asked before the build (which then writes the list of the
// rows outside the copy) and again by cauchy_wtd
bool wtdc_ready(lbfgsx_ctx* c, bool assume_defer)
{
    lbfgsb_state* b = c->bstate;
    const int total = 2 * c->ncorr;
    // the copy of the previous minimisation -- same history length (the commit replaced a slot) or one pair shorter (the commit
    // added one while the history fills: the copy's columns are slot-stable, wf_col, and the new pair is the "fresh" one of the
    // pass either way) -- not overgrown: the pass must read clearly less than the full-length one
    return b->wtdc_use && (b->corr_defer || assume_defer) && (b->split ? (total >= 2 && total <= kColsX) : (total > 8 && total <= 20)) &&
           !b->multidot_chunked && b->wf_use && b->wf_live &&
           (b->wf_ncorr == c->ncorr || b->wf_ncorr + 1 == c->ncorr) && b->wf_epoch == b->sub_epoch && c->n < (int64_t(1) << 31) &&
           b->wf_n >= 4096 && b->wf_n * 4 <= c->n * 3;
}
bool wtdc_prepare(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    b->wtdc_n = -1;
    if (!wtdc_ready(c))
        return false;
    return wtdc_alloc(c);
}
bool wtdc_alloc(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    if (!b->wtdc_list)
    {
        if (hipMalloc(reinterpret_cast<void**>(&b->wtdc_list), sizeof(int) * size_t(b->wtdc_cap)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&b->wtdc_cnt), sizeof(unsigned)) != hipSuccess ||
            hipMemsetAsync(b->wtdc_cnt, 0, sizeof(unsigned), c->stream) != hipSuccess)
        {
            (void) hipGetLastError();
            (void) hipFree(b->wtdc_list);
            (void) hipFree(b->wtdc_cnt);
            b->wtdc_list = nullptr;
            b->wtdc_cnt = nullptr;
            b->wtdc_use = false;
            return false;
        }
    }
    return true;
}

int run_force_bounds(lbfgsx_ctx* c)
{
    c->bstate->pb_valid = false;  // x may change: what the post pass computed ahead for the Cauchy search no longer holds
    lbfgsx::DeviceGuard dev_guard_(c->device);
    const int grid = c->grid_for(c->n);
    DISPATCH_T(c, {
        LBFGSX_LAUNCH((k_force_bounds<T>), dim3(grid), dim3(kBlock), 0, c->stream, P<T>(c->xb[c->cur]), P<T>(c->lb),
                           P<T>(c->ub), c->n);
    });
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}

int psort_alloc(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    if (!b->pk)
    {
        const size_t n = size_t(c->n);
        LBFGSX_HIP(hipMalloc(&b->pk, c->esz * n));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->pv), sizeof(int) * n));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->pcount), sizeof(unsigned)));
    }
    return LBFGSX_OK;
}

int delta_alloc(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    if (!b->fprev)
    {
        // room for n / 64 changed rows (what is worth patching instead of recomputing grows with n), 2^14 .. 2^20
        b->dl_cap = unsigned(std::min<int64_t>(c->n, std::max<int64_t>(int64_t(1) << 14, std::min<int64_t>(int64_t(1) << 20, c->n / 64))));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->fprev), size_t(c->ld)));   // padded like the state bytes
        LBFGSX_HIP(hipMemsetAsync(b->fprev, 0, size_t(c->ld), c->stream));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->dl_enter), sizeof(int) * size_t(b->dl_cap)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->dl_leave), sizeof(int) * size_t(b->dl_cap)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->dl_cnt), sizeof(unsigned) * 4));
    }
    return LBFGSX_OK;
}

}  // namespace lbfgsx

using namespace lbfgsx;

extern "C" {

int lbfgsx_b_reserve(lbfgsx_ctx* c)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    const int m2 = 2 * c->m;
    const int ncap = m2 <= 32 ? std::max(4, (m2 + 3) / 4 * 4) : m2 <= 40 ? 40 : m2 <= 48 ? 48 : m2 <= 64 ? 64 : 80;
    if (m2 <= 80)
    {
        rc = scan_alloc(c, std::min<int64_t>(int64_t(1) << 20, c->n), ncap);
        if (rc)
            return rc;
    }
    rc = psort_alloc(c);
    if (rc)
        return rc;
    rc = delta_alloc(c);
    if (rc)
        return rc;
    // the optional work sets: without room for them the passes that would use them do without
    if (b->wf_use && c->n >= 4096 && c->n < (int64_t(1) << 31))
        (void) wf_alloc(c);
    if (b->cv_use && b->wf_use)
        (void) cv_alloc(c);
    if (b->wtdc_use)
        (void) wtdc_alloc(c);
    return LBFGSX_OK;
}

int lbfgsx_b_compact_vec_counts(int64_t out[4], int reset)
{
    if (out)
    {
        out[0] = g_cv_starts.load(std::memory_order_relaxed);
        out[1] = g_cv_backs.load(std::memory_order_relaxed);
        out[2] = g_wtdc_runs.load(std::memory_order_relaxed);
        out[3] = g_stash_hits.load(std::memory_order_relaxed);
    }
    if (reset)
    {
        g_cv_starts = 0;
        g_cv_backs = 0;
        g_wtdc_runs = 0;
        g_stash_hits = 0;
    }
    return LBFGSX_OK;
}

int lbfgsx_b_set_compaction(lbfgsx_ctx* c, int enable)
{
    int rc = need_bounded(c);
    if (rc)
        return rc;
    c->bstate->wf_on = enable != 0;
    if (!enable)
        c->bstate->wf_valid = false;
    return LBFGSX_OK;
}

int lbfgsx_b_download_state(lbfgsx_ctx* c, unsigned char* host)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    LBFGSX_HIP(lbfgsx::copy_async(host, c->bstate->st, size_t(c->n), hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    return LBFGSX_OK;
}

// ---- inspection entries: the vectors of the subspace minimisation and the index list of L u U
static void* sub_vector(lbfgsb_state* b, int which)
{
    switch (which)
    {
    case LBFGSX_SV_CF: return b->cF;
    case LBFGSX_SV_Y: return b->y;
    case LBFGSX_SV_YFB: return b->yfb;
    case LBFGSX_SV_LAM: return b->lam;
    case LBFGSX_SV_MU: return b->mu;
    case LBFGSX_SV_RHS: return b->rhs;
    default: return nullptr;
    }
}
static int sub_copy(lbfgsx_ctx* c, int which, void* host, bool up)
{
    if (!c || !c->bstate || !host || !sub_vector(c->bstate, which))
    {
        set_error("lbfgsx_b_sub_download / _upload: needs a bounded context, a LBFGSX_SV_* selector and a host pointer");
        return LBFGSX_E_INVALID;
    }
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);  // live compact vectors are put back at their rows first
    if (rc)
        return rc;
    void* dev = sub_vector(c->bstate, which);
    const size_t bytes = size_t(c->n) * c->esz;
    if (up)
        LBFGSX_HIP(lbfgsx::copy_async(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    else
        LBFGSX_HIP(lbfgsx::copy_async(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    return LBFGSX_OK;
}

int lbfgsx_b_sub_download(lbfgsx_ctx* c, int which, void* host) { return sub_copy(c, which, host, false); }

int lbfgsx_b_sub_upload(lbfgsx_ctx* c, int which, const void* host) { return sub_copy(c, which, const_cast<void*>(host), true); }

int lbfgsx_b_lu_list_download(lbfgsx_ctx* c, int* rows, int64_t cap, int64_t* count)
{
    if (!c || !c->bstate || !count)
    {
        set_error("lbfgsx_b_lu_list_download: needs a bounded context and a count pointer");
        return LBFGSX_E_INVALID;
    }
    // reads only: the list's flags, the pending sweep and the compact vectors stay as they are
    const lbfgsb_state* b = c->bstate;
    if (!b->lu_valid)
    {
        *count = -1;
        return LBFGSX_OK;
    }
    if (cap < int64_t(b->lu_n) || (b->lu_n > 0 && !rows))
    {
        set_error("lbfgsx_b_lu_list_download: the list holds more rows than `cap`");
        return LBFGSX_E_INVALID;
    }
    lbfgsx::DeviceGuard dev_guard_(c->device);
    if (b->lu_n > 0)
    {
        LBFGSX_HIP(lbfgsx::copy_async(rows, b->lu_ptr(), sizeof(int) * size_t(b->lu_n), hipMemcpyDeviceToHost, c->stream));
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    }
    *count = b->lu_n;
    return LBFGSX_OK;
}

}  // extern "C"
