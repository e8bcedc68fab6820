// lbfgspp_amd/csrc/lbfgsb_state.hpp -- what the translation units of the L-BFGS-B device operators share (C ABI:
// include/lbfgsx.h, "L-BFGS-B" block): the per-context state, the pointer-bundle builders and the helpers more than one
// phase uses.  lbfgsb.hip (core: allocation, the shared helpers), lbfgsb_linesearch.hip, lbfgsb_dots.hip, lbfgsb_cauchy.hip,
// lbfgsb_gram.hip, lbfgsb_subspace.hip hold the entries of one phase each and the launchers only they use.
//
// Map of the per-context mechanisms kept in lbfgsb_state (each has an environment switch and a bit-identity test):
//   wf_*     compact copy of the free rows of the 2c columns (rows of F in order, idx / pos maps); written by the first
//            solve's Gram pass, kept and patched between iterations
//   cv_*     the vectors of the free rows by POSITION in that copy while a subspace minimisation sweeps (need_bounded's
//            keep_cv: the fused sweep entries work on them, every other entry gets them back at their rows first)
//   lu_*     index list of the rows of L u U of the last BOXCQP partition (ping-pong), dl_* rows that entered / left F
//   wtdc_*   rows outside the kept copy on which d or s_new is not zero: W'd of the Cauchy search over copy + list
//   psel_*   candidates of the partial break-point sort, listed by the Cauchy build itself
//   stash_*  Grams over index lists launched behind the pass before their request (need_bounded's keep_stash)
//   s_*, g_* buffers of the device / host form of the break-point search;  lbfgsx_b_reserve allocates all of it up front
// Round 4:
//   split    the passes over the 2c columns with a row's columns split over lane groups (lbfgsb_x.cuh / lbfgsb_x.hip, namespace
//            xl: any 2c <= 80); xp1, xp2, xtickets = the workspace of their grid reduction (reduce_x.cuh, wsx())
//   na_*     rows lbfgsx_b_cauchy_finish made newly active (a list for W_A'(A'd)); drt_ready: it also wrote drt = xcp - x0
//   pb_*     what the post statements' pass computed ahead for the Cauchy search (lbfgsx_b_post_linesearch_build) and the
//            state it assumed; lbfgsx_b_cauchy_build_partial uses it iff the solver is in that state
//   st_*     (ctx.hpp) the line search's first trial, evaluated by lbfgsx_b_dg_maxstep_trial; any bounded entry drops it
//   rhs_identity  a sweep's solve evaluates the rhs updates itself (lbfgsx_b_solve_sweep_rhs) and W_{L u U}'(-c) is delivered
//            un-rounded (lbfgsx_b_wtv_lu_c): BFGSMatB::solve_PtBP forms W_P' rhs on the host, no pass over P
// Waits: fetch_doubles / fetch_T / fetch_gram_out read host-mapped results after poll_wait (ctx.hpp) -- a polled completion
// word when the launch before them was armed (poll_arm), the stream otherwise.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ctx.hpp"
#include "lbfgsb_kernels.cuh"
#include "lbfgsb_x.hpp"

struct lbfgsb_state
{
    void *brk = nullptr, *dvec = nullptr, *cF = nullptr, *y = nullptr, *yfb = nullptr, *lam = nullptr, *mu = nullptr,
         *rhs = nullptr;
    unsigned char* st = nullptr;
    void *keys_in = nullptr, *keys_out = nullptr;
    int *vals_in = nullptr, *vals_out = nullptr;
    bool keys_valid = false;   // keys_in holds the sort keys of the break points in brk (a build may leave them out: ensure_keys)
    bool vals_iota = false;    // vals_in holds 0..n-1 (written by the first build, never changed by the sorts, which write vals_out)
    void* sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    int* phys_dev = nullptr;          // logical slot -> physical column, device copy
    unsigned phys_seen = 0;           //   ctx::phys_version that copy holds
    // lbfgsx_b_correction_dots_defer: the dots of the newest s against the history ride on the next W'd pass
    bool corr_defer = false, corr_stash_valid = false;
    double corr_raw[80];              //   raw dots (Y slots then S slots) kept for lbfgsx_b_correction_dots
    double* dout = nullptr;           // double outputs of the kernels [64]: device pointer of host-mapped memory, or
    double* dout_host = nullptr;      //   (LBFGSX_MAPPED_OUT=0) plain device memory fetched by a copy
    double* gram_out_host = nullptr;  // same for gram_out
    double* gram_dd = nullptr;        // [3][256][2] un-rounded (hi, lo) sums of the last one-pass Gram (device)
    double* gram_dd_host = nullptr;   // ... host-mapped when the mapped outputs are on (gram_dd is then its device alias)
    // Grams over index lists launched ahead of their request, behind a pass that is waited for anyway (one round trip less
    // each): slot 0 = rows of L u U (launched with lbfgsx_b_wtv_lu, asked for by the complement of the next solve), slots
    // 1, 2 = rows that entered / left the free set (launched with lbfgsx_b_gram_pairs_dd, asked for by
    // lbfgsx_b_gram_list_dd).  Host-mapped: [slot][3*256 rounded | 3*256*2 (hi, lo)].  Any other bounded entry drops them.
    double* stash_host = nullptr;
    double* stash_dev = nullptr;
    bool stash_use = true;            // LBFGSX_SYNC_MERGE=0: every Gram is launched when it is asked for
    bool stash_valid[3] = {false, false, false};
    bool stash_armed[3] = {false, false, false};  // launched, becomes valid with the launcher's wait
    unsigned stash_phys[3] = {0, 0, 0};
    int stash_tot[3] = {0, 0, 0};
    int64_t stash_hits = 0;
    void* coef_dev = nullptr;         // T[80]
    // index list of the rows the last BOXCQP partition put into L or U (k_sub_sweep_begin); lu_valid: it describes the
    // current state bytes (any other writer of ST_L / ST_U clears it)
    int* lu_list = nullptr;               // two buffers of lu_cap entries: the current list and the one a fused sweep builds
    int lu_cur = 0;
    int* lu_ptr() const { return lu_list + size_t(lu_cur) * size_t(lu_cap); }
    int* lu_other() const { return lu_list + size_t(1 - lu_cur) * size_t(lu_cap); }
    bool lu_pending = false;              // lbfgsx_b_solve_sweep(first = 0) ran; lbfgsx_b_lu_sweep completes the sweep
    int64_t lu_pending_n = 0;             //   rows that pass appended
    unsigned* lu_cnt = nullptr;
    unsigned lu_cap = 0;
    int lu_n = 0;
    int64_t lu_pred = int64_t(1) << 40;  // |L u U| of the previous partition: the list is only kept while the sets are small
    static constexpr int64_t kLuMax = 262144;  // ... i.e. up to this many rows (16384 until round 3: with 65536 .. 2^20
                                               // the iterations whose sets hold 10^4..10^5 rows keep the fused sweeps, +2 % from x0)
    bool lu_valid = false;
    bool sweep_fuse = true;               // LBFGSX_SWEEP_SOLVE_FUSE=0: the solve and the sweep's statements stay separate passes
    // compact copy of the free rows of [Y S] (GramRows, lbfgsb_kernels.cuh): written by the full Gram pass of the first
    // BOXCQP solve when the caller expects sweeps (lbfgsx_b_set_compaction), read by the passes of the sweeps
    void* wf = nullptr;                   // T[32][wf_ld]
    int64_t wf_ld = 0;
    int* wf_idx = nullptr;                // [n]
    int* wf_cnt = nullptr;                // [n / 64 + 2] free rows per batch, then their exclusive prefix
    int* wf_base = nullptr;
    void* wf_tmp = nullptr;
    size_t wf_tmp_bytes = 0;
    bool wf_use = true;                   // LBFGSX_COMPACT_FREE=0: never
    bool force_pending = false;           // lbfgsx_b_force_bounds_deferred: x = clamp(x) rides on the next Cauchy build
    // compact vectors of a subspace minimisation (lbfgsb_kernels.cuh "cv"): y, yfallback, lambda, mu, rhs, cF, lb - x0,
    // ub - x0 and the state byte of the free rows at their POSITION in the compact copy, from the first solve-sweep until
    // the result is assigned (or a pass outside the fused path needs them by row again: cv_back)
    // candidates of the partial break-point sort collected by the Cauchy build itself (k_cauchy_build's plist)
    // lbfgsx_b_post_linesearch_build: the Cauchy search's element-wise pass, taken by the pass of the post statements
    bool pb_use = true;                   // LBFGSX_POST_BUILD=0: two passes, as rounds 1-3
    bool st_use = true;                   // LBFGSX_TRIAL_AHEAD=0: lbfgsx_b_dg_maxstep_trial never evaluates the first trial ahead
    double vrow_dd[2 * 80];               // un-rounded (hi, lo) v row of the last full one-pass Gram (lbfgsx_b_gram_last_vrow_dd)
    bool vrow_dd_valid = false;
    bool rhs_identity = true;             // LBFGSX_RHS_IDENTITY=0: a sweep gets W_P'(-rhs) from a pass over P (kx_rows<NA = 1>), as before
    bool pb_valid = false;                // pb_r holds what k_cauchy_build would deliver for the state described below
    int pb_cur = -1;                      // the iterate buffer the pass read
    unsigned pb_writes = 0;               // ctx::vec_writes when the pass ran: an upload since then may have moved x, g or a bound
    double pb_tau = 0.0;
    bool pb_wc = false, pb_sel_inline = false;
    double pb_r[6] = {0, 0, 0, -1, -1, 0};  // d.d, #free, #ordered, #listed outside rows, #sort candidates | #rows the clamp moves
    bool psel_use = true;                 // LBFGSX_SELECT_INLINE=0: rocprim::select behind the build
    int* psel_list = nullptr;             // [psel_cap] rows in arrival order
    unsigned* psel_cnt = nullptr;
    unsigned psel_cap = 1u << 21;
    void* psel_tmp = nullptr;             // radix-sort workspace for psel_cap row numbers
    size_t psel_tmp_bytes = 0;
    int64_t psel_last = -1;               // candidates of the previous partial sort: the in-pass list pays while they are few
    bool list12 = true;                   // W_{L u U}'(-c) inside the pass that computes W_L'l and W_U'u (LBFGSX_LIST12=0: a launch of its own)
    bool psel_small = true;               // <= kPselSmallCap listed candidates: ordered by one block (LBFGSX_PSEL_SMALL=0: the three launches)
    static constexpr int64_t kPselMax = int64_t(1) << 17;  // candidates of the previous search up to which the build lists them
                                          // (appending and ordering 10^6 rows costs more than the separate selection pass)
    // W'd of the Cauchy search (and the deferred dots of add_correction) from the kept compact copy (k_multidot2_wf)
    bool wtdc_use = true;                 // LBFGSX_WTD_COMPACT=0: always the pass over the full-length columns
    int* wtdc_list = nullptr;             // rows outside the copy with d != 0 or s_new != 0 (k_cauchy_build)
    unsigned* wtdc_cnt = nullptr;
    unsigned wtdc_cap = 1u << 16;
    int64_t wtdc_n = -1;                  // entries of the list of this iteration's build; -1: none
    int64_t wtdc_runs = 0;
    bool cv_use = true;                   // LBFGSX_COMPACT_VEC=0: the vectors stay at their rows
    bool cv_live = false;
    void* cv_buf = nullptr;               // 8 vectors of cv_cap elements + cv_cap state bytes
    int64_t cv_cap = 0;
    int64_t cv_backs = 0, cv_starts = 0;  // instrumentation: passes that put them back early / minimisations that used them
    bool wf_on = false;                   // the caller's hint for the current subspace minimisation
    bool wf_valid = false;
    int64_t wf_n = 0;                     // rows in the copy
    int64_t nfree_last = 0;               // |F| of the last lbfgsx_b_cauchy_finish
    hipEvent_t chain_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // pieces of a Cauchy chunk
    static constexpr int kChainPieces = 8;  // a chunk of 2^17 crossings or more travels in this many pieces
    // rows that entered / left the free set since the last lbfgsx_b_free_delta (the carried Gram of BFGSMatB::solve_PtBP)
    unsigned char* fprev = nullptr;       // [n] free bit at that call
    int* dl_enter = nullptr;              // [dl_cap]
    int* dl_leave = nullptr;
    unsigned* dl_cnt = nullptr;           // [2]
    unsigned dl_cap = 0;
    int64_t dl_n[2] = {0, 0};             // rows in the two lists, -1: the list overflowed
    // the compact copy kept across iterations (the carried first solve): a superset of the free rows, every column current
    // except those the caller names when it uses it
    bool wf_live = false;
    int wf_ncorr = 0;                     // history size the copy's column order belongs to (Y slots, then S slots)
    // the kept copy is current only if the subspace minimisation right before this one wrote or patched it: one that did
    // neither (no sweeps expected, a fallback Gram, an early return) leaves a copy that misses that iteration's new columns
    long long sub_epoch = 0;              // subspace minimisations opened (lbfgsx_b_sub_begin)
    long long wf_epoch = -2;              // the one that last wrote or patched the copy
    long long wf_patched_epoch = -2;      // sub_epoch at which the W'd pass wrote the replaced pair into the copy ...
    int wf_patched_slot = -1;             // ... and the storage slot it wrote
    int* wf_pos = nullptr;                // [n] row -> position, -1: none
    double* g_host = nullptr;             // pinned landing zone of lbfgsx_b_cauchy_chunk
    // the first chunk of the sorted break points, gathered and copied behind the build's sort and ahead of its W'd pass: it
    // has landed when that pass's wait returns, and the host search's first lbfgsx_b_cauchy_chunk costs no round trip
    bool gpre_use = true;                 // LBFGSX_CHUNK_AHEAD=0
    // lbfgsx_b_free_delta launched ahead, behind the pass over the newly active rows (LBFGSX_DELTA_AHEAD=0: on request)
    bool fd_use = true, fd_ahead = false;
    long long fd_epoch = -1;
    unsigned* fd_host = nullptr;          // pinned: its four counters
    bool gpre_valid = false;
    int64_t gpre_count = 0;
    int gpre_nc = -1;
    size_t g_host_cap = 0;
    // chunk staging for the sequential GCP scan
    double *g_brk = nullptr, *g_g = nullptr, *g_z = nullptr, *g_w = nullptr;
    int* g_idx = nullptr;
    int64_t g_cap = 0;
    int g_ncorr = 0;
    double* gram_partial = nullptr;   // [kGramBlocks][3][256][2]
    double* gram_partial2 = nullptr;  // [32][3][256][2]
    double* gram_out = nullptr;       // [3][256]
    static constexpr int kGramBlocks = 1024;  // 4 resident blocks per CU (33 KB of LDS each)
    // exact Gram on the matrix cores (gram_i8.cuh): radix-256 digits, v_mfma_i32_32x32x32_i8, integer sums
    bool gram_i8 = false;                    // LBFGSX_GRAM=i8
    int i8_min_tot = 1;                      // fewer columns than this: the double-double kernel (LBFGSX_GRAM_I8_MIN)
    unsigned long long* colmax = nullptr;    // [m + 1][2]: bit patterns of max |Y col|, max |S col| per physical column
    std::vector<unsigned char> colmax_ok;    // per physical column: the slots above describe the column's current content
    long long* i8_part = nullptr;            // [waves][11][ne_pad]
    double* i8_partv = nullptr;              // [waves][32][2]
    unsigned long long* i8_vsum = nullptr;   // [11][ne_pad]
    int i8_waves = 0, i8_nepad = 0;
    int gram_mode = 0;       // 2 (LBFGSX_GRAM=blocked): force the multi-launch blocked Gram + separate W'v
    int num_cus = 256;
    static constexpr int kDotsGrid = 512;  // blocks of the all-column multi-dot kernels
    bool multidot_chunked = false;  // LBFGSX_MULTIDOT=chunked: 8 columns per launch (round-1a kernel)
    // device GCP search (gcp_scan.cuh): per-chunk work set, allocated on first use
    double *s_brk = nullptr, *s_g = nullptr, *s_z = nullptr, *s_W = nullptr, *s_P = nullptr, *s_C = nullptr,
           *s_fpp = nullptr, *s_dfp = nullptr, *s_fp = nullptr, *s_ts = nullptr, *s_off = nullptr, *s_small = nullptr;
    unsigned long long* s_exit = nullptr;
    // host-order chain (chain_host): the exit index goes to k_gcp_extract and its 2 NC + 4 results come back through
    // host-mapped memory instead of a copy each way (three copies fewer per scan call)
    unsigned long long* exit_map_host = nullptr;
    unsigned long long* exit_map_dev = nullptr;
    double* gout_host = nullptr;
    double* gout_dev = nullptr;
    double* s_chain = nullptr;  // s_fp | s_dfp | s_fpp in ONE allocation, laid out per call with pitch count + 1
    double* h_chain = nullptr;   // pinned: [3][s_cap + 1] per-crossing terms of the f' / f'' chains (exact-order mode)
    bool chain_host = true;      // LBFGSX_GCP_CHAIN=scan: tree-order f' / f'' on the device instead
    int64_t s_cap = 0;
    int s_nc = 0;
    // partial sort of the break points (lbfgsx_b_cauchy_build_partial): compacted candidates, allocated on first use
    void* pk = nullptr;
    int* pv = nullptr;
    unsigned* pcount = nullptr;
    void* sel_tmp = nullptr;
    size_t sel_tmp_bytes = 0;
    // the passes for any history length (lbfgsb_x.cuh: a row's columns split over the lanes of a wavefront)
    bool split = true;                // LBFGSX_SPLIT=0: the one-lane-per-row kernels of round 3 where they exist (2c <= 20 / 24 / 32)
    double* xp1 = nullptr;            // workspace of grid_reduce_x: per-block and per-group partials, tickets
    double* xp2 = nullptr;
    unsigned* xtickets = nullptr;
    int gtile = 3;                    // 256-entry tiles the Gram buffers hold: >= (2m + 1)(2m + 2) / 2 entries
    // lbfgsx_b_cauchy_finish also evaluates drt = xcp - x0 (the statement lbfgsx_b_sub_begin would run next) and lists the rows
    // it made newly active; both hold until another bounded entry runs (need_bounded's keep_fin)
    bool fin_fuse = true;             // LBFGSX_FINISH_FUSE=0: the separate passes
    bool drt_ready = false;
    int* na_list = nullptr;           // [na_cap] newly active rows, in arrival order
    unsigned* na_cnt = nullptr;
    unsigned na_cap = 1u << 16;
    int64_t na_n = -1;                // entries of the list, -1: none / overflowed
    int64_t na_prev = -1;             // rows the previous search made newly active (-1: no search yet): the list is only asked for
                                      // when that fitted it -- a search that activates millions of rows (the first iterations)
                                      // otherwise has 10^5 waves meeting at one counter for a list nobody reads
    static constexpr int kDout = 640; // doubles of `dout`
};

// copies of these files carry their file and line in the host trace (LBFGSX_HOST_TRACE; scripts/host_trace.py); every
// translation unit names itself (LBFGSB_TU, its file stem) before it includes this header
#define copy_async(...) copy_async_at("copy@" LBFGSB_TU ":" LBFGSX_STR(__LINE__), __VA_ARGS__)

namespace lbfgsx {

#define DISPATCH_T(c, ...)            \
    do                                \
    {                                 \
        if ((c)->dtype == LBFGSX_F64) \
        {                             \
            typedef double T;         \
            __VA_ARGS__               \
        }                             \
        else                          \
        {                             \
            typedef float T;          \
            __VA_ARGS__               \
        }                             \
    } while (0)

template <class T>
inline T* P(void* p) { return static_cast<T*>(p); }

template <class T>
inline BVecs<T> bvecs(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    BVecs<T> v;
    v.x0 = P<T>(c->xb[c->cur]);
    v.g = P<T>(c->gb[c->cur]);
    v.lb = P<T>(c->lb);
    v.ub = P<T>(c->ub);
    v.xcp = P<T>(c->xcp);
    v.drt = P<T>(c->d);
    v.brk = P<T>(b->brk);
    v.dvec = P<T>(b->dvec);
    v.cF = P<T>(b->cF);
    v.y = P<T>(b->y);
    v.yfb = P<T>(b->yfb);
    v.lam = P<T>(b->lam);
    v.mu = P<T>(b->mu);
    v.rhs = P<T>(b->rhs);
    v.st = b->st;
    return v;
}

// the vectors of the free rows by POSITION (cv_buf): what the fused sweep kernels are handed while cv_live
template <class T>
inline BVecs<T> bvecs_cv(lbfgsx_ctx* c, T** cli = nullptr, T** cui = nullptr)
{
    lbfgsb_state* b = c->bstate;
    BVecs<T> v = bvecs<T>(c);
    T* base = static_cast<T*>(b->cv_buf);
    const int64_t cap = b->cv_cap;
    v.y = base;
    v.yfb = base + cap;
    v.lam = base + 2 * cap;
    v.mu = base + 3 * cap;
    v.rhs = base + 4 * cap;
    v.cF = base + 5 * cap;
    if (cli) *cli = base + 6 * cap;
    if (cui) *cui = base + 7 * cap;
    v.st = reinterpret_cast<unsigned char*>(base + 8 * cap);
    return v;
}

// logical-slot column pointer lists
template <class T, int NC>
inline Cols<T, NC> col_list(lbfgsx_ctx* c, const int* which /* 0..2c-1: Y slots then S slots */, int count)
{
    Cols<T, NC> cl;
    for (int k = 0; k < NC; k++)
    {
        if (k < count)
        {
            const int w = which[k];
            const int slot = (w < c->ncorr) ? w : w - c->ncorr;
            void* base = (w < c->ncorr) ? c->Y : c->S;
            cl.p[k] = static_cast<const T*>(c->col(base, c->phys[size_t(slot)]));
        }
        else
            cl.p[k] = cl.p[0];  // padding: valid memory, so that a kernel may load all NC columns without a branch per column
    }
    return cl;
}

// Column of the compact copy that holds logical column k (Y slots, then S slots) of a history of `count / 2` pairs: slot-stable
// (round 5) -- Y slot j in column j, S slot j in column m + j whatever the history length, so that a copy written while the
// history fills stays valid when the next pair arrives (only the new slot's two columns are missing: the patch of the
// carried Gram's pass).  Until round 4 the S slots followed the Y slots directly and every new pair moved them.
inline int wf_col(const lbfgsx_ctx* c, int k, int count)
{
    const int cc = count / 2;
    return k < cc ? k : c->m + (k - cc);
}
// columns of the compact copy of the free rows, logical order (Y slots then S slots)
template <class T>
inline Cols<T, 32> wf_cols(lbfgsx_ctx* c, int count)
{
    Cols<T, 32> cl;
    for (int k = 0; k < 32; k++)
        cl.p[k] = static_cast<const T*>(c->bstate->wf) + int64_t(wf_col(c, k < count ? k : 0, count)) * c->bstate->wf_ld;  // padded with column 0
    return cl;
}
// the same lists for the kernels of lbfgsb_x.cuh (2c <= 80), and the workspace of their reductions
template <class T>
inline ColsX<T> colsx_full(lbfgsx_ctx* c, int count)
{
    ColsX<T> cl;
    for (int k = 0; k < kColsX; k++)
    {
        const int w = (k < count) ? k : 0;
        const int slot = (w < c->ncorr) ? w : w - c->ncorr;
        void* base = (w < c->ncorr) ? c->Y : c->S;
        cl.p[k] = static_cast<const T*>(c->col(base, c->phys[size_t(slot)]));
    }
    return cl;
}
template <class T>
inline ColsX<T> colsx_wf(lbfgsx_ctx* c, int count)
{
    ColsX<T> cl;
    for (int k = 0; k < kColsX; k++)
        cl.p[k] = static_cast<const T*>(c->bstate->wf) + int64_t(wf_col(c, k < count ? k : 0, count)) * c->bstate->wf_ld;
    return cl;
}
// a mask inside the free set can be served from the compact copy
inline bool wf_serves(const lbfgsx_ctx* c, int mask)
{
    return c->bstate->wf_valid && mask != 0 && (mask & ~(ST_FREE | ST_L | ST_U | ST_P)) == 0;
}

// ---- lbfgsb.hip (core) ----
// keep_force: the caller is the Cauchy build, which evaluates a deferred x = clamp(x) itself (lbfgsx_b_force_bounds_deferred);
// every other entry of the bounded path runs it first
// keep_cv: the caller is one of the fused sweep entries, which work on the compact vectors of the free rows; every other
// entry gets them back at their rows first
// keep_stash: the caller launches or consumes the Grams launched ahead (lbfgsb_state::stash_*); any other entry may change
// what they were computed from and drops them
// keep_fin: the caller is one of the two entries that follow lbfgsx_b_cauchy_finish and use what it left (drt_ready, na_*)
int need_bounded(lbfgsx_ctx* c, bool keep_force = false, bool keep_cv = false, bool keep_stash = false, bool keep_fin = false);
int upload_phys(lbfgsx_ctx* c);
int fetch_doubles(lbfgsx_ctx* c, int k, double* out);
template <class T>
int fetch_T(lbfgsx_ctx* c, int idx, int k, double* out);  // instantiated for float and double
RedWsX wsx(lbfgsx_ctx* c);
int ensure_keys(lbfgsx_ctx* c);
int cv_alloc(lbfgsx_ctx* c);
int cv_back(lbfgsx_ctx* c, bool assign);
int run_force_bounds(lbfgsx_ctx* c);
void wf_rebuilt(lbfgsx_ctx* c);
bool wtdc_ready(lbfgsx_ctx* c, bool assume_defer = false);
bool wtdc_prepare(lbfgsx_ctx* c);
bool wtdc_alloc(lbfgsx_ctx* c);
int psort_alloc(lbfgsx_ctx* c);
int delta_alloc(lbfgsx_ctx* c);
// the process-wide counters of lbfgsx_b_compact_vec_counts, for the phases that count
void count_cv_start();
void count_wtdc_run();
void count_stash_hit();
// ---- lbfgsb_linesearch.hip ----
void count_pb_hit();  // lbfgsx_b_post_build_counts: a Cauchy build took what the post pass computed ahead
// ---- lbfgsb_dots.hip: the two doors to the multi-dot kernels (element type from c->dtype) ----
int wtv(lbfgsx_ctx* c, int vsel_id, const void* vcol, int mask, double* out, int64_t* nnz);
int cauchy_wtd(lbfgsx_ctx* c, double* wtd);
// ---- lbfgsb_cauchy.hip: the one translation unit with rocprim (the sorts, the selection, the scan that places the batches
// of the compact copy) and with gcp_scan.cuh ----
bool wf_alloc(lbfgsx_ctx* c);
bool wf_prepare(lbfgsx_ctx* c);
size_t sort_pairs_tmp_bytes(lbfgsx_ctx* c);  // workspace of the radix sort of all n (break point, row) pairs
bool psel_alloc(lbfgsx_ctx* c);
int scan_alloc(lbfgsx_ctx* c, int64_t count, int NC);
// ---- lbfgsb_gram.hip ----
int free_delta_launch(lbfgsx_ctx* c);
bool gram_stash_feasible(lbfgsx_ctx* c, const int* list, int64_t nlist);
bool gram_stash_launch(lbfgsx_ctx* c, int slot, int mask, const int* list, int64_t nlist, bool signal = false);
void gram_stash_settle(lbfgsx_ctx* c, bool ok);
}  // namespace lbfgsx
