// lbfgspp_amd/csrc/lbfgsb_gram.hip -- L-BFGS-B device operators, the Grams W_P'W_P: blocked, one-pass double-double, exact integer (gram_i8.cuh),
// over index lists and launched ahead (stash), single rows (k_vrows), and the free-set delta the carried Gram is patched with.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#include "gram_i8.cuh"

#define LBFGSB_TU "lbfgsb_gram"
#include "lbfgsb_state.hpp"

namespace lbfgsx {

int bounded_note_column(lbfgsx_ctx* c, int col)
{
    lbfgsb_state* b = c->bstate;
    if (!b || !b->gram_i8 || col < 0 || col > c->m)
        return LBFGSX_OK;
    unsigned long long* cmx = b->colmax + 2 * size_t(col);
    LBFGSX_HIP(hipMemsetAsync(cmx, 0, 2 * sizeof(unsigned long long), c->stream));
    const int grid = c->grid_for(c->n);
    DISPATCH_T(c, {
        LBFGSX_LAUNCH((k_colmax2<T>), dim3(grid), dim3(kBlock), 0, c->stream, P<T>(c->col(c->S, col)), P<T>(c->col(c->Y, col)),
                           c->n, cmx + 1, cmx + 0);
    });
    LBFGSX_HIP(hipGetLastError());
    b->colmax_ok[size_t(col)] = 1;
    return LBFGSX_OK;
}

// exact integer Gram on the matrix cores (gram_i8.cuh): returns the number of per-wave partials, or -1 when not applicable
// compact: the pass walks the compact copy of the free rows (wf_cols, wf_n rows, row list wf_idx) instead of the full-length
// columns under the mask -- the same rows, the same integer sums
template <int CS>
static int launch_gram_i8_cs(lbfgsx_ctx* c, int tot, int vsel_id, int mask, const GramPrologue<double>& pro, const GramI8Args& ga,
                             int blocks, int ne_pad, bool compact)
{
    lbfgsb_state* b = c->bstate;
    int which[32];
    for (int k = 0; k < tot; k++)
        which[k] = k;
    Cols<double, 32> cl = compact ? wf_cols<double>(c, tot) : col_list<double, 32>(c, which, tot);
    const size_t lds = size_t(kBlock / 64) * kI8Ring * size_t(CS) * sizeof(double);
    LBFGSX_LAUNCH((k_gram_i8<CS>), dim3(blocks), dim3(kBlock), lds, c->stream, cl, tot, bvecs<double>(c), vsel_id, mask,
                  compact ? b->wf_n : c->n, b->i8_part, ne_pad, b->i8_partv, pro, ga,
                  compact ? b->wf_idx : static_cast<const int*>(nullptr));
    return blocks * (kBlock / 64);
}
// compact_out: the pass (over the full-length columns) also writes the compact copy of the free rows (wf_prepare done)
static int gram_i8_run(lbfgsx_ctx* c, int tot, int vsel_id, int mask, const GramPrologue<double>& pro, bool want_dd, bool compact,
                       bool compact_out)
{
    lbfgsb_state* b = c->bstate;
    GramI8Args ga;
    ga.colmax = b->colmax;
    ga.out_w = compact_out ? static_cast<double*>(b->wf) : nullptr;
    ga.out_ld = b->wf_ld;
    ga.out_split = c->ncorr;   // slot-stable columns of the copy (wf_col)
    ga.out_gap = c->m - c->ncorr;
    ga.out_idx = b->wf_idx;
    ga.out_base = b->wf_base;
    ga.out_pos = b->wf_pos;
    for (int k = 0; k < 32; k++)
        ga.cidx[k] = 0;
    for (int k = 0; k < tot; k++)
    {
        const int slot = (k < c->ncorr) ? k : k - c->ncorr;
        const int col = c->phys[size_t(slot)];
        if (!b->colmax_ok[size_t(col)])
            return -1;
        ga.cidx[k] = 2 * col + ((k < c->ncorr) ? 0 : 1);  // Y columns first, then S columns (col_list's order)
    }
    const int ne = tot * (tot + 1) / 2;
    const int ne_pad = (ne + 63) / 64 * 64;
    const int64_t nbatch = ((compact ? b->wf_n : c->n) + kGramDDRows - 1) / kGramDDRows;
    const int blocks = int(std::max<int64_t>(1, std::min<int64_t>(b->num_cus, (nbatch + 3) / 4)));
    const int waves = blocks * (kBlock / 64);
    if (waves > b->i8_waves || ne_pad > b->i8_nepad)
    {
        (void) hipFree(b->i8_part);
        (void) hipFree(b->i8_partv);
        (void) hipFree(b->i8_vsum);
        b->i8_part = nullptr;
        b->i8_partv = nullptr;
        b->i8_vsum = nullptr;
        const int wcap = std::max(waves, b->num_cus * (kBlock / 64));
        const int ecap = std::max(ne_pad, 512);  // 2c <= 30 -> 465 entries
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->i8_part), sizeof(long long) * size_t(wcap) * kI8Acc * size_t(ecap)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->i8_partv), sizeof(double) * size_t(wcap) * 32 * 2));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->i8_vsum), sizeof(unsigned long long) * kI8Acc * size_t(ecap)));
        b->i8_waves = wcap;
        b->i8_nepad = ecap;
    }
    LBFGSX_HIP(hipMemsetAsync(b->i8_vsum, 0, sizeof(unsigned long long) * kI8Acc * size_t(ne_pad), c->stream));
    LBFGSX_HIP(hipMemsetAsync(b->i8_part, 0, sizeof(long long) * size_t(blocks) * kI8Acc * size_t(ne_pad), c->stream));
    if (vsel_id >= 0)
        LBFGSX_HIP(hipMemsetAsync(b->i8_partv, 0, sizeof(double) * size_t(waves) * 32 * 2, c->stream));
    if (tot <= 23)
        launch_gram_i8_cs<23>(c, tot, vsel_id, mask, pro, ga, blocks, ne_pad, compact);
    else
        launch_gram_i8_cs<31>(c, tot, vsel_id, mask, pro, ga, blocks, ne_pad, compact);
    LBFGSX_LAUNCH(k_gram_i8_sum, dim3(kI8Acc, std::min(blocks, 16)), dim3(kBlock), 0, c->stream, b->i8_part, blocks, ne, ne_pad,
                       b->i8_vsum);
    LBFGSX_LAUNCH(k_gram_i8_final, dim3(1), dim3(kBlock), 0, c->stream, b->i8_vsum, tot, ne_pad, b->i8_partv, waves,
                       vsel_id >= 0 ? 1 : 0, ga, b->gram_out, want_dd ? b->gram_dd : static_cast<double*>(nullptr));
    LBFGSX_HIP(hipGetLastError());
    return waves;
}

template <class T, int KP>
static int launch_gram_dd(lbfgsx_ctx* c, int64_t nbatch, int tot, int vsel_id, int mask, const GramPrologue<T>& pro,
                          const GramRows<T>& gr, int64_t nrows)
{
    lbfgsb_state* b = c->bstate;
    const size_t lds = gram_dd_lds_bytes(gram_dd_cs(KP), KP);
    // one persistent wave set per resident slot: occupancy x CUs blocks (3 per CU at m = 10)
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_gram_dd<T, KP>, kBlock, lds) != hipSuccess || occ < 1)
        occ = 2;
    int blocks = std::min(lbfgsb_state::kGramBlocks, occ * b->num_cus);
    blocks = int(std::max<int64_t>(1, std::min<int64_t>(blocks, (nbatch + 3) / 4)));
    int which[32];
    for (int k = 0; k < tot; k++)
        which[k] = k;
    Cols<T, 32> cl = (gr.in_idx && !gr.w_by_row) ? wf_cols<T>(c, tot) : col_list<T, 32>(c, which, tot);
    // byte model: state bytes (and row numbers) of every row walked, the columns and v of the rows kept (nrows), the compact copy when written
    lbfgsx::model_add(double(nbatch) * 64.0 * (1 + (gr.in_idx ? 4 : 0)) +
                      double((!gr.in_idx && mask && b->nfree_last > 0) ? std::min<int64_t>(nrows, b->nfree_last) : nrows) * sizeof(T) *
                          (tot * (gr.out_w ? 2 : 1) + 1));
    LBFGSX_LAUNCH((k_gram_dd<T, KP>), dim3(blocks), dim3(kBlock), lds, c->stream, cl, tot, bvecs<T>(c), vsel_id, mask,
                       nrows, b->gram_partial, pro, gr);
    return blocks;
}
template <class T, int CS>
static int launch_gram_vonly(lbfgsx_ctx* c, int64_t nbatch, int tot, int vsel_id, int mask, const GramPrologue<T>& pro,
                             const GramRows<T>& gr, int64_t nrows)
{
    lbfgsb_state* b = c->bstate;
    const size_t lds = gram_dd_lds_bytes(CS, 1);
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_gram_dd<T, 1, CS, true>, kBlock, lds) != hipSuccess || occ < 1)
        occ = 2;
    int blocks = std::min(lbfgsb_state::kGramBlocks, occ * b->num_cus);
    blocks = int(std::max<int64_t>(1, std::min<int64_t>(blocks, (nbatch + 3) / 4)));
    int which[32];
    for (int k = 0; k < tot; k++)
        which[k] = k;
    Cols<T, 32> cl = (gr.in_idx && !gr.w_by_row) ? wf_cols<T>(c, tot) : col_list<T, 32>(c, which, tot);
    // byte model: state bytes (and row numbers) of every row walked, the columns and v of the rows kept (nrows), the compact copy when written
    lbfgsx::model_add(double(nbatch) * 64.0 * (1 + (gr.in_idx ? 4 : 0)) +
                      double((!gr.in_idx && mask && b->nfree_last > 0) ? std::min<int64_t>(nrows, b->nfree_last) : nrows) * sizeof(T) *
                          (tot * (gr.out_w ? 2 : 1) + 1));
    LBFGSX_LAUNCH((k_gram_dd<T, 1, CS, true>), dim3(blocks), dim3(kBlock), lds, c->stream, cl, tot, bvecs<T>(c), vsel_id,
                       mask, nrows, b->gram_partial, pro, gr);
    return blocks;
}
// A Gram over the rows of an index list (2c x 2c, no v row) launched ahead of its request into stash slot `slot`; mask != 0:
// only the listed rows whose state byte has one of its bits.  false: not launched (the request will launch it itself).
constexpr int64_t kListOneBlock = 512 * kGramSelfFinish;  // rows of a list whose Gram ONE kx_gram launch forms and finishes (<= 512 per block)
static inline int list_blocks(int64_t nlist) { return int(std::max<int64_t>(1, std::min<int64_t>(kGramSelfFinish, (nlist + 127) / 128))); }
bool gram_stash_feasible(lbfgsx_ctx* c, const int* list, int64_t nlist)
{
    lbfgsb_state* b = c->bstate;
    const int tot = 2 * c->ncorr;
    return b->stash_use && b->stash_host && b->gram_mode != 2 && tot >= 1 && (tot <= kGramDDCS || b->split) && list &&
           nlist >= 1;
}
// signal: this is the last launch before the caller's wait -- its final block carries the completion word (ctx.hpp)
bool gram_stash_launch(lbfgsx_ctx* c, int slot, int mask, const int* list, int64_t nlist, bool signal)
{
    lbfgsb_state* b = c->bstate;
    const int tot = 2 * c->ncorr;
    b->stash_valid[slot] = b->stash_armed[slot] = false;
    if (!gram_stash_feasible(c, list, nlist))
        return false;
    if (upload_phys(c) != LBFGSX_OK)
        return false;
    const int npairs = tot * (tot + 1) / 2;
    const int kp = (npairs + 63) / 64;
    const int kpt = kp <= 1 ? 1 : kp <= 2 ? 2 : kp <= 4 ? 4 : kp <= 6 ? 6 : 8;
    const int ntile = (64 * kpt + 255) / 256;
    const int64_t nbatch = (nlist + kGramDDRows - 1) / kGramDDRows;
    int blocks = 1;
    double* out = b->stash_dev + size_t(slot) * (size_t(b->gtile) * 256 * 3);
    const bool single = b->split && nlist <= kListOneBlock;
    if (tot > kGramDDCS || single)
    {
        // the block-tile kernel (lbfgsb_x.cuh): more columns than the wave-private tiles hold, or a list short enough for ONE
        // block, whose launch then leaves the finished sums itself (no kx_gram_finish launches: one launch instead of three)
        int rcx = LBFGSX_OK;
        double* out_dd = out + size_t(b->gtile) * 256;
        if (signal && single)
            lbfgsx::poll_arm(c);
        DISPATCH_T(c, {
            ProX<T> pro{};
            pro.mode = LBFGSX_GP_NONE;
            GramRows<T> gr{};
            gr.in_idx = list;
            gr.w_by_row = 1;
            if (b->cv_live)
            {
                gr.st_alt = bvecs_cv<T>(c).st;
                gr.st_pos = b->wf_pos;
            }
            blocks = xl::gram<T>(c->stream, single ? list_blocks(nlist) : lbfgsb_state::kGramBlocks, colsx_full<T>(c, tot),
                                 tot, bvecs<T>(c), -1, mask, nlist, b->gram_partial, pro, gr, out, out_dd,
                                 (signal && single) ? c->ws.done : static_cast<unsigned long long*>(nullptr),
                                 (signal && single) ? c->ws.seq : 0ull, b->xtickets + 1 + kMaxGridX / kGroupX);
        });
        if (blocks < 1)
            return false;
        if (blocks > kGramSelfFinish)
        {
            const int nt = xl::gram_kpb(tot);
            if (signal)
                lbfgsx::poll_arm(c);
            rcx = xl::gram_finish(c->stream, b->gram_partial, blocks, nt, b->gram_partial2, out, out_dd,
                                  signal ? c->ws.done : static_cast<unsigned long long*>(nullptr), signal ? c->ws.seq : 0ull,
                                  b->xtickets + 1 + kMaxGridX / kGroupX);
        }
        if (rcx != LBFGSX_OK)
            return false;
        b->stash_armed[slot] = true;
        b->stash_phys[slot] = c->phys_version;
        b->stash_tot[slot] = tot;
        return true;
    }
    DISPATCH_T(c, {
        GramPrologue<T> pro;
        pro.mode = LBFGSX_GP_NONE;
        pro.use1 = pro.use2 = 0;
        for (int k = 0; k < 64; k++)
            pro.c1[k] = pro.c2[k] = T(0);
        GramRows<T> gr{};
        gr.in_idx = list;
        gr.w_by_row = 1;
        if (b->cv_live)
        {
            gr.st_alt = bvecs_cv<T>(c).st;
            gr.st_pos = b->wf_pos;
        }
        if (kp <= 1) blocks = launch_gram_dd<T, 1>(c, nbatch, tot, -1, mask, pro, gr, nlist);
        else if (kp <= 2) blocks = launch_gram_dd<T, 2>(c, nbatch, tot, -1, mask, pro, gr, nlist);
        else if (kp <= 4) blocks = launch_gram_dd<T, 4>(c, nbatch, tot, -1, mask, pro, gr, nlist);
        else if (kp <= 6) blocks = launch_gram_dd<T, 6>(c, nbatch, tot, -1, mask, pro, gr, nlist);
        else blocks = launch_gram_dd<T, 8>(c, nbatch, tot, -1, mask, pro, gr, nlist);
    });
    const int nch = std::min(blocks, 32);
    LBFGSX_LAUNCH(k_gram_finish, dim3(ntile, nch), dim3(kBlock), 0, c->stream, b->gram_partial, blocks, b->gram_partial2, 0);
    if (signal && ntile == 1)
        lbfgsx::poll_arm(c);
    else
        signal = false;
    LBFGSX_LAUNCH(k_gram_finish, dim3(ntile, 1), dim3(kBlock), 0, c->stream, b->gram_partial2, nch, out, 1, out + size_t(b->gtile) * 256,
                  signal ? c->ws.done : static_cast<unsigned long long*>(nullptr), signal ? c->ws.seq : 0ull);
    if (hipGetLastError() != hipSuccess)
        return false;
    b->stash_armed[slot] = true;
    b->stash_phys[slot] = c->phys_version;
    b->stash_tot[slot] = tot;
    return true;
}
// after the launcher's wait: what was launched ahead is there (ok) or never will be
void gram_stash_settle(lbfgsx_ctx* c, bool ok)
{
    lbfgsb_state* b = c->bstate;
    for (int q = 0; q < 3; q++)
    {
        b->stash_valid[q] = ok && b->stash_armed[q];
        b->stash_armed[q] = false;
    }
}
// the (hi, lo) sums of slot `slot` if they are what the caller is about to compute
static bool gram_stash_take(lbfgsx_ctx* c, int slot, double* gram, double* gram_dd)
{
    lbfgsb_state* b = c->bstate;
    const int tot = 2 * c->ncorr;
    const bool hit = b->stash_valid[slot] && b->stash_phys[slot] == c->phys_version && b->stash_tot[slot] == tot;
    b->stash_valid[slot] = false;
    if (!hit)
        return false;
    const double* h = b->stash_host + size_t(slot) * (size_t(b->gtile) * 256 * 3);
    if (gram)
        for (int i = 0; i < tot; i++)
            for (int j = 0; j <= i; j++)
            {
                const double v = h[i * (i + 1) / 2 + j];
                gram[i * tot + j] = v;
                gram[j * tot + i] = v;
            }
    if (gram_dd)
        std::memcpy(gram_dd, h + size_t(b->gtile) * 256, sizeof(double) * size_t(tot) * size_t(tot + 1));
    b->stash_hits++;
    count_stash_hit();
    return true;
}

// k_vrows: the v row (NA = 1) or the v row and the rows of two columns (NA = 3) of the masked Gram, rounded values in
// gram_out[r * (NC + 1) + j] and (hi, lo) pairs from gram_out + 256 on (host-mapped when the mapped outputs are on)
template <class T, int NC, int NA>
static int launch_vrows(lbfgsx_ctx* c, int tot, int vsel_id, int mask, const GramPrologue<T>& pro, const GramRows<T>& gr,
                        int64_t nrows, int col_a, int col_b, const BVecs<T>* by_pos = nullptr)
{
    // by_pos: the compact vectors are live -- the rows of the compact copy in order, their vectors at the same positions
    lbfgsb_state* b = c->bstate;
    int which[32];
    for (int k = 0; k < tot; k++)
        which[k] = k;
    Cols<T, 32> cl = (gr.in_idx || by_pos) ? wf_cols<T>(c, tot) : col_list<T, 32>(c, which, tot);
    // resident wave sets: two blocks per CU while the accumulators leave room for two waves per SIMD, else one
    const int per_cu = (NA == 1 && NC <= 20) ? 2 : 1;
    const int grid = std::max(1, std::min(std::min(c->grid_for(nrows), b->num_cus * per_cu), c->ws.maxGrid));
    LBFGSX_LAUNCH((k_vrows<T, NC, NA>), dim3(grid), dim3(kBlock), 0, c->stream, cl, tot, by_pos ? *by_pos : bvecs<T>(c), vsel_id,
                  mask, nrows, c->ws, b->gram_out, b->gram_out + 256, pro, gr, col_a, col_b);
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}
template <class T>
static int launch_vrows_v(lbfgsx_ctx* c, int tot, int vsel_id, int mask, const GramPrologue<T>& pro, const GramRows<T>& gr,
                          int64_t nrows, const BVecs<T>* by_pos = nullptr)
{
    if (tot <= 8) return launch_vrows<T, 8, 1>(c, tot, vsel_id, mask, pro, gr, nrows, 0, 0, by_pos);
    if (tot <= 16) return launch_vrows<T, 16, 1>(c, tot, vsel_id, mask, pro, gr, nrows, 0, 0, by_pos);
    if (tot <= 20) return launch_vrows<T, 20, 1>(c, tot, vsel_id, mask, pro, gr, nrows, 0, 0, by_pos);
    if (tot <= 24) return launch_vrows<T, 24, 1>(c, tot, vsel_id, mask, pro, gr, nrows, 0, 0, by_pos);
    return launch_vrows<T, 32, 1>(c, tot, vsel_id, mask, pro, gr, nrows, 0, 0, by_pos);
}
// the (hi, lo) outputs of k_vrows (and its rounded values) on the host: `count` doubles from gram_out + first
static int fetch_gram_out(lbfgsx_ctx* c, int first, int count, double* h)
{
    lbfgsb_state* b = c->bstate;
    if (b->gram_out_host)
    {
        LBFGSX_HIP(lbfgsx::poll_wait(c));
        const volatile double* src = b->gram_out_host + first;
        for (int i = 0; i < count; i++)
            h[i] = src[i];
        return LBFGSX_OK;
    }
    LBFGSX_HIP(lbfgsx::copy_async(h, b->gram_out + first, sizeof(double) * size_t(count), hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    return LBFGSX_OK;
}
// Can the requested entries be served by k_vrows?  Every entry must lie in the v row (I = tot) or contain one of at most
// two other columns (the two columns add_correction replaced, in the carried first solve).  slot[z] = index of entry z
// in the kernel's output, rows of NP entries: 0 = v row, 1 = column a, 2 = column b.
static bool vrows_plan(int npairs, const int* pi, const int* pj, int tot, int NP, int& col_a, int& col_b, int* slot)
{
    int freq[kColsX + 1];
    for (int k = 0; k <= kColsX; k++)
        freq[k] = 0;
    bool other = false;
    for (int z = 0; z < npairs; z++)
        if (pi[z] != tot && pj[z] != tot)
        {
            other = true;
            freq[pi[z]]++;
            if (pj[z] != pi[z])
                freq[pj[z]]++;
        }
    col_a = col_b = -1;
    if (other)
    {
        for (int k = 0; k < tot; k++)
            if (col_a < 0 || freq[k] > freq[col_a])
                col_a = k;
        for (int k = 0; k < tot; k++)
            if (k != col_a && freq[k] > 0 && (col_b < 0 || freq[k] > freq[col_b]))
                col_b = k;
        if (col_b < 0)
            col_b = col_a;
    }
    for (int z = 0; z < npairs; z++)
    {
        const int I = pi[z], J = pj[z];
        if (I == tot || J == tot)
            slot[z] = (I == tot) ? J : I;                       // v row: entry = the other index (tot for v.v)
        else if (I == col_a || J == col_a)
            slot[z] = NP + (I == col_a ? J : I);
        else if (I == col_b || J == col_b)
            slot[z] = 2 * NP + (I == col_b ? J : I);
        else
            return false;
    }
    return true;
}
// everything of lbfgsx_b_free_delta up to the copy of its four counters into pinned memory (fd_host); nothing is waited for
int free_delta_launch(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    int rc = delta_alloc(c);
    if (rc)
        return rc;
    if (!b->fd_host)
        LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->fd_host), sizeof(unsigned) * 4, hipHostMallocDefault));
    // (a history that has grown by the one pair of this iteration keeps the copy: its columns are slot-stable, wf_col; the new
    // slot's two columns are the patch of the carried Gram's pass)
    if (b->wf_live && (!(b->wf_ncorr == c->ncorr || b->wf_ncorr + 1 == c->ncorr) || b->wf_epoch + 1 != b->sub_epoch))
        b->wf_live = false;  // the copy missed an iteration (or the history was reset)
    // {rows entered, rows left, rows in the kept compact copy, 1: the copy cannot be kept}
    const unsigned init[4] = {0u, 0u, unsigned(b->wf_live ? b->wf_n : 0), 0u};
    LBFGSX_HIP(lbfgsx::copy_async(b->dl_cnt, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    const int64_t n8 = (c->n + 7) / 8;
    const int grid = c->grid_for(n8);
    lbfgsx::model_add(double(c->n) * 2.125);  // byte model: the state bytes read, the remembered free bits read and written
    LBFGSX_LAUNCH(k_free_delta, dim3(grid), dim3(kBlock), 0, c->stream, b->st, b->fprev, n8, c->n, b->dl_enter, b->dl_leave,
                       b->dl_cnt, b->dl_cap);
    LBFGSX_HIP(hipGetLastError());
    if (b->wf_live)
    {
        // rows new to the free set join the kept compact copy
        rc = upload_phys(c);
        if (rc)
            return rc;
        const int total = 2 * c->ncorr;
        int which[kColsX];
        for (int k = 0; k < total; k++)
            which[k] = k;
        DISPATCH_T(c, {
            if (total > 32)
                (void) xl::wf_append<T>(c->stream, colsx_full<T>(c, total), total, static_cast<T*>(b->wf), b->wf_ld, b->wf_idx, b->wf_pos,
                                        b->dl_enter, b->dl_cnt, b->dl_cap, unsigned(std::min<int64_t>(c->n, b->wf_ld)), c->ncorr,
                                        c->m - c->ncorr);
            else
            {
            Cols<T, 32> cl = col_list<T, 32>(c, which, total);
            LBFGSX_LAUNCH((k_wf_append<T>), dim3(16), dim3(kBlock), 0, c->stream, cl, total, static_cast<T*>(b->wf), b->wf_ld,
                               b->wf_idx, b->wf_pos, b->dl_enter, b->dl_cnt, b->dl_cap, unsigned(std::min<int64_t>(c->n, b->wf_ld)),
                               c->ncorr, c->m - c->ncorr);
            }
        });
        LBFGSX_HIP(hipGetLastError());
    }
    LBFGSX_HIP(lbfgsx::copy_async(b->fd_host, b->dl_cnt, sizeof(unsigned) * 4, hipMemcpyDeviceToHost, c->stream));
    return LBFGSX_OK;
}
// list != nullptr: the Gram over the nlist rows of an index list (mask ignored, full-length columns read at those rows)
static int gram_dd_core(lbfgsx_ctx* c, int mask, int vsel_id, int prologue, const double* coef1, const double* coef2,
                        double* gram, double* wtv, double* gram_dd, const int* list, int64_t nlist)
{
    int rc = need_bounded(c, false, /*keep_cv=*/true, /*keep_stash=*/true);  // the walk over the L u U list reads the partition bits where they are
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    b->vrow_dd_valid = false;
    const int tot = 2 * c->ncorr;
    const int ntot = tot + (vsel_id >= 0 ? 1 : 0);
    const bool lu_walk = !list && b->lu_valid && vsel_id < 0 && prologue == LBFGSX_GP_NONE && mask != 0 &&
                         (mask & ~(ST_L | ST_U)) == 0;
    // launched ahead?  (slot 0: the rows of L u U behind lbfgsx_b_wtv_lu; slots 1, 2: the entered / left rows behind
    // lbfgsx_b_gram_pairs_dd)
    {
        int slot = -1;
        if (lu_walk && mask == (ST_L | ST_U) && b->lu_n >= 1)
            slot = 0;
        else if (list && vsel_id < 0 && prologue == LBFGSX_GP_NONE && list == b->dl_enter)
            slot = 1;
        else if (list && vsel_id < 0 && prologue == LBFGSX_GP_NONE && list == b->dl_leave)
            slot = 2;
        const bool hit = slot >= 0 && !wtv && gram_stash_take(c, slot, gram, gram_dd);
        if (slot != 0)  // the sweeps may ask for the L u U Gram only right after lbfgsx_b_wtv_lu
            b->stash_valid[0] = false;
        if (hit)
            return LBFGSX_OK;
    }
    if (b->cv_live && !lu_walk)
    {
        rc = cv_back(c, false);
        if (rc)
            return rc;
    }
    if (prologue != LBFGSX_GP_NONE && (prologue < 0 || prologue > LBFGSX_GP_LINEAR))
    {
        set_error("lbfgsx_b_gram_fused_ex: the prologue needs the default one-pass Gram");
        return LBFGSX_E_INVALID;
    }
    // kx_gram, the block-tile kernel: 2c + 1 > 31, and (decided below) short row lists, which one block finishes by itself
    bool wide = ntot > kGramDDCS && b->split;
    if (tot < 1 || (ntot > kGramDDCS && !wide) || b->gram_mode == 2)
    {
        set_error("lbfgsx_b_gram_fused: one-pass Gram not applicable");
        return LBFGSX_E_INVALID;
    }
    std::vector<double> hbuf(size_t(b->gtile) * 256);
    double* h = hbuf.data();
    const int npairs = ntot * (ntot + 1) / 2;
    const int kp = (npairs + 63) / 64;  // pairs per lane: 1, 2, 4, 6 or 8 (ntot <= 31 -> 496 pairs)
    int blocks = 1;
    rc = upload_phys(c);
    if (rc)
        return rc;
    // the pass over the whole free set that keeps its un-rounded sums is the first solve of a subspace minimisation: with
    // sweeps expected it also leaves the compact copy of the free rows (worth it when F leaves out a good part of the rows)
    if (list)
        mask = 0;
    else if (lu_walk)
    {
        // the complement Gram of a BOXCQP sweep (rows of L u U): walk the index list of the partition instead of the state
        // bytes of every (free) row; the mask stays, the list may hold rows of the other set
        if (b->lu_n < 1)
        {
            if (gram)
                std::fill(gram, gram + size_t(tot) * size_t(tot), 0.0);
            if (gram_dd)
                std::fill(gram_dd, gram_dd + size_t(tot) * size_t(tot + 1), 0.0);
            return LBFGSX_OK;
        }
        list = b->lu_ptr();
        nlist = b->lu_n;
    }
    const bool compact_in = !list && wf_serves(c, mask);
    bool compact_out = !list && !compact_in && b->wf_use && b->wf_on && gram_dd != nullptr && mask == ST_FREE && vsel_id >= 0 &&
                       c->n < (int64_t(1) << 31) && b->nfree_last >= 4096 && b->nfree_last * 8 <= c->n * 7;
    if (compact_out)
        compact_out = wf_prepare(c);
    const int64_t nrows = list ? nlist : compact_in ? b->wf_n : c->n;
    const int64_t nbatch = (nrows + kGramDDRows - 1) / kGramDDRows;
    bool done_i8 = false;
    // the integer kernel pays a fixed cost per launch (per-wave partials, the integer tree): row sets that are not the
    // free set -- the sparse L u U complements of the BOXCQP sweeps -- stay on the double-double kernel
    if (!list && b->gram_i8 && c->dtype == LBFGSX_F64 && tot <= 30 && tot >= b->i8_min_tot && (mask == 0 || (mask & ST_FREE)))
    {
        GramPrologue<double> pro;
        pro.mode = prologue;
        pro.use1 = coef1 ? 1 : 0;
        pro.use2 = coef2 ? 1 : 0;
        for (int k = 0; k < 64; k++)
        {
            pro.c1[k] = (coef1 && k < tot) ? coef1[k] : 0.0;
            pro.c2[k] = (coef2 && k < tot) ? coef2[k] : 0.0;
        }
        const int w = gram_i8_run(c, tot, vsel_id, mask, pro, gram_dd != nullptr, compact_in, compact_out);
        if (w < -1)
            return w;
        done_i8 = (w > 0);
        if (done_i8 && compact_out)
            wf_rebuilt(c);
    }
    const int kpt_ = kp <= 1 ? 1 : kp <= 2 ? 2 : kp <= 4 ? 4 : kp <= 6 ? 6 : 8;
    const bool one_block = list && b->split && !b->gram_i8 && nlist <= kListOneBlock && prologue == LBFGSX_GP_NONE;
    wide = wide || one_block;
    const int ntile_ = wide ? xl::gram_kpb(ntot) : (64 * kpt_ + 255) / 256;
    if (wide)
    {
        DISPATCH_T(c, {
            ProX<T> pro;
            pro.mode = prologue;
            pro.use1 = coef1 ? 1 : 0;
            pro.use2 = coef2 ? 1 : 0;
            for (int k = 0; k < kColsX; k++)
            {
                pro.c1[k] = (coef1 && k < tot) ? T(coef1[k]) : T(0);
                pro.c2[k] = (coef2 && k < tot) ? T(coef2[k]) : T(0);
            }
            GramRows<T> gr{};
            gr.in_idx = list ? list : compact_in ? b->wf_idx : nullptr;
            gr.w_by_row = list ? 1 : 0;
            if (b->cv_live)  // lu_walk
            {
                gr.st_alt = bvecs_cv<T>(c).st;
                gr.st_pos = b->wf_pos;
            }
            if (compact_out)
            {
                gr.out_w = static_cast<T*>(b->wf);
                gr.out_ld = b->wf_ld;
            gr.out_split = c->ncorr;   // slot-stable columns of the copy (wf_col)
            gr.out_gap = c->m - c->ncorr;
                gr.out_idx = b->wf_idx;
                gr.out_base = b->wf_base;
                gr.out_pos = b->wf_pos;
            }
            const ColsX<T> cl = (gr.in_idx && !gr.w_by_row) ? colsx_wf<T>(c, tot) : colsx_full<T>(c, tot);
            blocks = xl::gram<T>(c->stream, one_block ? list_blocks(nrows) : lbfgsb_state::kGramBlocks, cl, tot, bvecs<T>(c),
                                 vsel_id, mask, nrows, b->gram_partial, pro, gr, b->gram_out,
                                 gram_dd ? b->gram_dd : static_cast<double*>(nullptr), nullptr, 0ull,
                                 one_block ? b->xtickets + 1 + kMaxGridX / kGroupX : static_cast<unsigned*>(nullptr));
        });
        if (blocks < 1)
        {
            set_error("lbfgsx_b_gram_fused: kx_gram launch failed");
            return LBFGSX_E_HIP;
        }
        if (compact_out)
            wf_rebuilt(c);
        if (blocks > kGramSelfFinish || !one_block)
        {
            rc = xl::gram_finish(c->stream, b->gram_partial, blocks, ntile_, b->gram_partial2, b->gram_out,
                                 gram_dd ? b->gram_dd : static_cast<double*>(nullptr), nullptr, 0ull,
                                 b->xtickets + 1 + kMaxGridX / kGroupX);
            if (rc)
                return rc;
        }
    }
    else if (!done_i8)
    {
    DISPATCH_T(c, {
        GramPrologue<T> pro;
        pro.mode = prologue;
        pro.use1 = coef1 ? 1 : 0;
        pro.use2 = coef2 ? 1 : 0;
        for (int k = 0; k < 64; k++)
        {
            pro.c1[k] = (coef1 && k < tot) ? T(coef1[k]) : T(0);
            pro.c2[k] = (coef2 && k < tot) ? T(coef2[k]) : T(0);
        }
        GramRows<T> gr{};
        gr.in_idx = list ? list : compact_in ? b->wf_idx : nullptr;
        gr.w_by_row = list ? 1 : 0;
        if (b->cv_live)  // lu_walk
        {
            gr.st_alt = bvecs_cv<T>(c).st;
            gr.st_pos = b->wf_pos;
        }
        if (compact_out)
        {
            gr.out_w = static_cast<T*>(b->wf);
            gr.out_ld = b->wf_ld;
            gr.out_split = c->ncorr;   // slot-stable columns of the copy (wf_col)
            gr.out_gap = c->m - c->ncorr;
            gr.out_idx = b->wf_idx;
            gr.out_base = b->wf_base;
            gr.out_pos = b->wf_pos;
        }
        if (kp <= 1) blocks = launch_gram_dd<T, 1>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
        else if (kp <= 2) blocks = launch_gram_dd<T, 2>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
        else if (kp <= 4) blocks = launch_gram_dd<T, 4>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
        else if (kp <= 6) blocks = launch_gram_dd<T, 6>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
        else blocks = launch_gram_dd<T, 8>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
    });
    if (compact_out)
        wf_rebuilt(c);
    const int nch = std::min(blocks, 32);
    LBFGSX_LAUNCH(k_gram_finish, dim3(ntile_, nch), dim3(kBlock), 0, c->stream, b->gram_partial, blocks, b->gram_partial2, 0);
    LBFGSX_LAUNCH(k_gram_finish, dim3(ntile_, 1), dim3(kBlock), 0, c->stream, b->gram_partial2, nch, b->gram_out, 1,
                       gram_dd ? b->gram_dd : static_cast<double*>(nullptr));
    LBFGSX_HIP(hipGetLastError());
    }
    const int ntile = ntile_;
    std::vector<double> hdd;
    if (gram_dd && !b->gram_dd_host)
    {
        hdd.resize(size_t(ntile) * 256 * 2);
        LBFGSX_HIP(lbfgsx::copy_async(hdd.data(), b->gram_dd, sizeof(double) * hdd.size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (b->gram_out_host)
    {
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
        std::memcpy(h, b->gram_out_host, sizeof(double) * size_t(ntile) * 256);
    }
    else
    {
        LBFGSX_HIP(lbfgsx::copy_async(h, b->gram_out, sizeof(double) * size_t(ntile) * 256, hipMemcpyDeviceToHost, c->stream));
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    }
    if (gram)
        for (int i = 0; i < tot; i++)
            for (int j = 0; j <= i; j++)
            {
                const double v = h[i * (i + 1) / 2 + j];
                gram[i * tot + j] = v;
                gram[j * tot + i] = v;
            }
    if (wtv && vsel_id >= 0)
        for (int j = 0; j < tot; j++)
            wtv[j] = h[tot * (tot + 1) / 2 + j];
    if (gram_dd)  // packed lower triangle of the 2c x 2c block, e = i (i + 1) / 2 + j: (hi, lo)
        std::memcpy(gram_dd, b->gram_dd_host ? b->gram_dd_host : hdd.data(), sizeof(double) * size_t(tot) * size_t(tot + 1));
    if (gram_dd && wtv && vsel_id >= 0 && !list)  // the v row of the same tile, un-rounded: entries e = tot (tot + 1) / 2 + j (the integer kernel
                                                  // leaves its exact sums in the same places)
    {
        const double* dd = b->gram_dd_host ? b->gram_dd_host : hdd.data();
        std::memcpy(b->vrow_dd, dd + size_t(tot) * size_t(tot + 1), sizeof(double) * size_t(2 * tot));
        b->vrow_dd_valid = true;
    }
    return LBFGSX_OK;
}

}  // namespace lbfgsx

using namespace lbfgsx;

extern "C" {

int lbfgsx_b_gram(lbfgsx_ctx* c, int mask, double* gram)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    // lower triangle (and everything else, by symmetry) of the 2c x 2c Gram of [Y_P, S_P] in logical slot order
    int rc = need_bounded(c);
    if (rc)
        return rc;
    constexpr int TB = 4;
    const int tot = 2 * c->ncorr;
    const int grid = c->grid_for(c->n);
    for (int bi = 0; bi < tot; bi += TB)
        for (int bj = 0; bj <= bi; bj += TB)
        {
            const int ni = std::min(TB, tot - bi), nj = std::min(TB, tot - bj);
            int wi[TB], wj[TB];
            for (int k = 0; k < ni; k++)
                wi[k] = bi + k;
            for (int k = 0; k < nj; k++)
                wj[k] = bj + k;
            double r[TB * TB];
            DISPATCH_T(c, {
                Cols<T, TB> ci = col_list<T, TB>(c, wi, ni), cj = col_list<T, TB>(c, wj, nj);
                LBFGSX_LAUNCH((k_gram<T, TB>), dim3(grid), dim3(kBlock), 0, c->stream, ci, ni, cj, nj, c->bstate->st, mask,
                                   c->n, c->ws, c->bstate->dout);
            });
            LBFGSX_HIP(hipGetLastError());
            rc = fetch_doubles(c, TB * TB, r);
            if (rc)
                return rc;
            for (int a = 0; a < ni; a++)
                for (int b2 = 0; b2 < nj; b2++)
                {
                    gram[(bi + a) * tot + (bj + b2)] = r[a * TB + b2];
                    gram[(bj + b2) * tot + (bi + a)] = r[a * TB + b2];
                }
        }
    return LBFGSX_OK;
}

int lbfgsx_b_wtv_prologue(lbfgsx_ctx* c, int mask, int vsel_id, int prologue, const double* coef1, const double* coef2,
                          double* wtv)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, false, /*keep_cv=*/true);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    const int tot = 2 * c->ncorr, ntot = tot + 1;
    const bool xsplit = b->split;  // kx_rows: any 2c <= 80
    if (tot < 1 || (ntot > kGramDDCS && !xsplit) || tot > kColsX || vsel_id < 0 || !wtv || b->gram_mode == 2 ||
        prologue < LBFGSX_GP_NONE || prologue > LBFGSX_GP_LINEAR)
    {
        set_error("lbfgsx_b_wtv_prologue: needs the default one-pass Gram, 1 <= 2c <= 80, a vector selector and a known prologue");
        return LBFGSX_E_INVALID;
    }
    // the compact vectors serve the pass between two sweeps: rhs += ..., v = -rhs on the P rows of the compact copy
    const bool by_pos = b->cv_live && wf_serves(c, mask) && prologue != LBFGSX_GP_LINEAR &&
                        (vsel_id == VS_NEG_RHS || vsel_id == VS_NEG_CF || vsel_id == VS_Y);
    if (b->cv_live && !by_pos)
    {
        rc = cv_back(c, false);
        if (rc)
            return rc;
    }
    const bool compact = wf_serves(c, mask);
    const int64_t nrows = compact ? b->wf_n : c->n;
    rc = upload_phys(c);
    if (rc)
        return rc;
    if (xsplit)
    {
        DISPATCH_T(c, {
            ProX<T> pro;
            pro.mode = prologue;
            pro.use1 = coef1 ? 1 : 0;
            pro.use2 = coef2 ? 1 : 0;
            for (int k = 0; k < kColsX; k++)
            {
                pro.c1[k] = (coef1 && k < tot) ? T(coef1[k]) : T(0);
                pro.c2[k] = (coef2 && k < tot) ? T(coef2[k]) : T(0);
            }
            RowsX<T> gr{};
            gr.in_idx = (compact && !by_pos) ? b->wf_idx : nullptr;
            const BVecs<T> cvb = bvecs_cv<T>(c);
            const ColsX<T> cl = (gr.in_idx || by_pos) ? colsx_wf<T>(c, tot) : colsx_full<T>(c, tot);
            lbfgsx::poll_arm(c);
            rc = xl::rows<T>(c->stream, b->num_cus, 1, cl, tot, by_pos ? cvb : bvecs<T>(c), vsel_id, mask, nrows, wsx(c), b->gram_out,
                             b->gram_out + 256, pro, gr, -1, -1);
        });
        if (rc)
            return rc;
        double hx[kColsX];
        rc = fetch_gram_out(c, 0, tot, hx);
        if (rc)
            return rc;
        for (int j = 0; j < tot; j++)
            wtv[j] = hx[j];
        return LBFGSX_OK;
    }
    DISPATCH_T(c, {
        GramPrologue<T> pro;
        pro.mode = prologue;
        pro.use1 = coef1 ? 1 : 0;
        pro.use2 = coef2 ? 1 : 0;
        for (int k = 0; k < 64; k++)
        {
            pro.c1[k] = (coef1 && k < tot) ? T(coef1[k]) : T(0);
            pro.c2[k] = (coef2 && k < tot) ? T(coef2[k]) : T(0);
        }
        GramRows<T> gr{};
        gr.in_idx = (compact && !by_pos) ? b->wf_idx : nullptr;
        const BVecs<T> cvb = bvecs_cv<T>(c);
        lbfgsx::poll_arm(c);
        rc = launch_vrows_v<T>(c, tot, vsel_id, mask, pro, gr, nrows, by_pos ? &cvb : nullptr);
    });
    if (rc)
        return rc;
    double h[64];
    rc = fetch_gram_out(c, 0, tot, h);  // k_vrows: the last block has published the rounded sums
    if (rc)
        return rc;
    for (int j = 0; j < tot; j++)
        wtv[j] = h[j];
    return LBFGSX_OK;
}

int lbfgsx_b_free_delta(lbfgsx_ctx* c, int64_t* n_enter, int64_t* n_leave)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    // launched ahead, behind the pass over the newly active rows (lbfgsx_b_wtv), for this subspace minimisation?  Then its
    // counters landed with that pass's wait
    const bool ahead = b->fd_ahead && b->fd_epoch == b->sub_epoch;
    b->fd_ahead = false;
    if (!ahead)
    {
        rc = free_delta_launch(c);
        if (rc)
            return rc;
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    }
    const unsigned* h = b->fd_host;
    for (int d = 0; d < 2; d++)
        b->dl_n[d] = (h[d] <= b->dl_cap) ? int64_t(h[d]) : -1;
    if (b->wf_live)
    {
        if (h[3])
            b->wf_live = false;
        else
            b->wf_n = int64_t(h[2]);
    }
    *n_enter = b->dl_n[0];
    *n_leave = b->dl_n[1];
    return LBFGSX_OK;
}

int lbfgsx_b_gram_list_dd(lbfgsx_ctx* c, int which, double* gram_dd)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, false, false, /*keep_stash=*/true);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    if (which < 0 || which > 1 || !b->fprev || b->dl_n[which] < 1 || !gram_dd)
    {
        set_error("lbfgsx_b_gram_list_dd: no such list (lbfgsx_b_free_delta first; an overflowed or empty list has no Gram)");
        return LBFGSX_E_INVALID;
    }
    return gram_dd_core(c, 0, -1, LBFGSX_GP_NONE, nullptr, nullptr, nullptr, nullptr, gram_dd, which == 0 ? b->dl_enter : b->dl_leave,
                        b->dl_n[which]);
}

int lbfgsx_b_gram_pairs_max(lbfgsx_ctx* c)
{
    if (!c || !c->bstate)
        return 0;
    const lbfgsb_state* b = c->bstate;
    const int tot = 2 * c->ncorr;
    if (tot < 1 || tot > kColsX || b->gram_mode == 2)
        return 0;
    if (b->split)
        return 3 * (tot + 1);
    return tot + 1 <= kGramDDCS ? 64 : 0;
}

int lbfgsx_b_gram_pairs_dd(lbfgsx_ctx* c, int mask, int vsel_id, int prologue, const double* coef1, const double* coef2,
                           int npairs, const int* pair_i, const int* pair_j, int refresh_slot, double* out_dd)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    const int tot = 2 * c->ncorr, ntot = tot + 1;
    const bool xsplit = b->split;  // kx_rows: any 2c <= 80, up to 3 (2c + 1) entries
    if (tot < 1 || tot > kColsX || vsel_id < 0 || !out_dd || b->gram_mode == 2 || npairs < 1 ||
        (xsplit ? npairs > 3 * (kColsX + 1) : (npairs > 64 || ntot > kGramDDCS)) || prologue < LBFGSX_GP_NONE || prologue > LBFGSX_GP_LINEAR)
    {
        set_error("lbfgsx_b_gram_pairs_dd: needs the default one-pass Gram, 1 <= 2c <= 80, a vector selector and 1..3 (2c + 1) entries");
        return LBFGSX_E_INVALID;
    }
    for (int e = 0; e < npairs; e++)
        if (pair_i[e] < 0 || pair_i[e] > tot || pair_j[e] < 0 || pair_j[e] > tot)
        {
            set_error("lbfgsx_b_gram_pairs_dd: entry outside the [Y S v] columns");
            return LBFGSX_E_INVALID;
        }
    if (refresh_slot < -2 || refresh_slot >= c->ncorr)
    {
        set_error("lbfgsx_b_gram_pairs_dd: refresh_slot is a storage slot, -1 (nothing replaced) or -2 (no kept copy)");
        return LBFGSX_E_INVALID;
    }
    // the copy kept from the previous iteration serves when the caller vouches for the history (refresh_slot >= -1), the
    // mask is the free set and the copy is not overgrown with rows that have left it
    const bool same_hist = b->wf_ncorr == c->ncorr || (b->wf_ncorr + 1 == c->ncorr && refresh_slot == c->ncorr - 1);
    const bool kept = refresh_slot >= -1 && b->wf_live && b->wf_use && mask == ST_FREE && b->wf_n * 8 <= b->nfree_last * 9 &&
                      b->wf_n >= b->nfree_last && same_hist && b->wf_epoch + 1 == b->sub_epoch;
    if (!kept)
        b->wf_live = false;
    const bool compact_in = kept || wf_serves(c, mask);
    bool compact_out = !compact_in && b->wf_use && b->wf_on && mask == ST_FREE &&
                       c->n < (int64_t(1) << 31) && b->nfree_last >= 4096 && b->nfree_last * 8 <= c->n * 7;
    rc = upload_phys(c);
    if (rc)
        return rc;
    if (compact_out)
        compact_out = wf_prepare(c);
    const int64_t nrows = compact_in ? b->wf_n : c->n;
    const int64_t nbatch = (nrows + kGramDDRows - 1) / kGramDDRows;
    int blocks = 1;
    // the register kernel serves the pass that writes no new copy when the entries are the v row plus the rows of at most
    // two columns (3 (2c + 1) <= 64 sums: one lane per sum in the block reduction)
    int col_a = -1, col_b = -1, slot[3 * (kColsX + 1)];
    bool ride_enter = false, ride_leave = false;
    if (xsplit)
    {
        // the v row plus the rows of at most two columns, whatever 2c is; a pass that must also write a new compact copy is
        // the full Gram's business (the caller falls back to it)
        if (compact_out || !vrows_plan(npairs, pair_i, pair_j, tot, tot + 1, col_a, col_b, slot))
        {
            if (ntot > kGramDDCS || npairs > 64)
            {
                set_error("lbfgsx_b_gram_pairs_dd: these entries need the full pass");
                return LBFGSX_E_INVALID;
            }
        }
        else
        {
            DISPATCH_T(c, {
                ProX<T> pro;
                pro.mode = prologue;
                pro.use1 = coef1 ? 1 : 0;
                pro.use2 = coef2 ? 1 : 0;
                for (int k = 0; k < kColsX; k++)
                {
                    pro.c1[k] = (coef1 && k < tot) ? T(coef1[k]) : T(0);
                    pro.c2[k] = (coef2 && k < tot) ? T(coef2[k]) : T(0);
                }
                RowsX<T> gr{};
                gr.in_idx = compact_in ? b->wf_idx : nullptr;
                // (the W'd pass of this iteration may have written the replaced pair into the copy already: wtd2_wf_x)
                const bool prepatched = b->wf_patched_epoch + 1 == b->sub_epoch && b->wf_patched_slot == refresh_slot;
                if (kept && refresh_slot >= 0 && !prepatched)
                {
                    gr.fresh_a = refresh_slot;
                    gr.fresh_b = c->ncorr + refresh_slot;
                    gr.src_a = static_cast<const T*>(c->col(c->Y, c->phys[size_t(refresh_slot)]));
                    gr.src_b = static_cast<const T*>(c->col(c->S, c->phys[size_t(refresh_slot)]));
                    gr.dst_a = static_cast<T*>(b->wf) + int64_t(wf_col(c, gr.fresh_a, 2 * c->ncorr)) * b->wf_ld;
                    gr.dst_b = static_cast<T*>(b->wf) + int64_t(wf_col(c, gr.fresh_b, 2 * c->ncorr)) * b->wf_ld;
                }
                ride_enter = b->fprev && b->dl_n[0] >= 1 && gram_stash_feasible(c, b->dl_enter, b->dl_n[0]);
                ride_leave = b->fprev && b->dl_n[1] >= 1 && gram_stash_feasible(c, b->dl_leave, b->dl_n[1]);
                if (!ride_enter && !ride_leave)
                    lbfgsx::poll_arm(c);
                const ColsX<T> cl = compact_in ? colsx_wf<T>(c, tot) : colsx_full<T>(c, tot);
                // the three-row form also patches the two replaced columns of the kept copy (the one-row form never does)
                rc = xl::rows<T>(c->stream, b->num_cus, (col_a < 0 && !gr.dst_a) ? 1 : 3, cl, tot, bvecs<T>(c), vsel_id, mask, nrows,
                                 wsx(c), b->gram_out, b->gram_out + 256, pro, gr, col_a, col_b);
            });
            if (kept)
            {
                b->wf_valid = true;  // usable by the passes of this subspace minimisation
                b->wf_epoch = b->sub_epoch;
                b->wf_ncorr = c->ncorr;  // (a pair that arrived since the copy was written has been patched in)
            }
            if (rc)
                return rc;
            if (ride_enter)
                (void) gram_stash_launch(c, 1, 0, b->dl_enter, b->dl_n[0], /*signal=*/!ride_leave);
            if (ride_leave)
                (void) gram_stash_launch(c, 2, 0, b->dl_leave, b->dl_n[1], /*signal=*/true);
            double hx[2 * 3 * (kColsX + 1)];
            rc = fetch_gram_out(c, 256, 2 * 3 * (tot + 1), hx);
            gram_stash_settle(c, rc == LBFGSX_OK);
            if (rc)
                return rc;
            for (int z = 0; z < npairs; z++)
            {
                out_dd[2 * z] = hx[2 * slot[z]];
                out_dd[2 * z + 1] = hx[2 * slot[z] + 1];
            }
            return LBFGSX_OK;
        }
    }
    bool use_vrows = !compact_out && vrows_plan(npairs, pair_i, pair_j, tot, (tot <= 20 ? 20 : 32) + 1, col_a, col_b, slot);
    if (use_vrows && col_a >= 0 && (tot > 20 || !compact_in))  // the three-row form walks the compact copy's row list
        use_vrows = false;
    if (use_vrows && col_a < 0)  // v row only: the row length of the class launch_vrows_v picks
    {
        const int np = (tot <= 8 ? 8 : tot <= 16 ? 16 : tot <= 20 ? 20 : tot <= 24 ? 24 : 32) + 1;
        (void) vrows_plan(npairs, pair_i, pair_j, tot, np, col_a, col_b, slot);
    }
    DISPATCH_T(c, {
        GramPrologue<T> pro;
        pro.mode = prologue;
        pro.use1 = coef1 ? 1 : 0;
        pro.use2 = coef2 ? 1 : 0;
        for (int k = 0; k < 64; k++)
        {
            pro.c1[k] = (coef1 && k < tot) ? T(coef1[k]) : T(0);
            pro.c2[k] = (coef2 && k < tot) ? T(coef2[k]) : T(0);
        }
        GramRows<T> gr{};
        gr.in_idx = compact_in ? b->wf_idx : nullptr;
        gr.vgroups = 1;
        gr.use_table = 1;
        if (compact_out)
        {
            gr.out_w = static_cast<T*>(b->wf);
            gr.out_ld = b->wf_ld;
            gr.out_split = c->ncorr;   // slot-stable columns of the copy (wf_col)
            gr.out_gap = c->m - c->ncorr;
            gr.out_idx = b->wf_idx;
            gr.out_base = b->wf_base;
            gr.out_pos = b->wf_pos;
        }
        if (kept && refresh_slot >= 0)
        {
            gr.fresh_a = refresh_slot;
            gr.fresh_b = c->ncorr + refresh_slot;
            gr.src_a = static_cast<const T*>(c->col(c->Y, c->phys[size_t(refresh_slot)]));
            gr.src_b = static_cast<const T*>(c->col(c->S, c->phys[size_t(refresh_slot)]));
            gr.dst_a = static_cast<T*>(b->wf) + int64_t(wf_col(c, gr.fresh_a, 2 * c->ncorr)) * b->wf_ld;
            gr.dst_b = static_cast<T*>(b->wf) + int64_t(wf_col(c, gr.fresh_b, 2 * c->ncorr)) * b->wf_ld;
        }
        for (int e = 0; e < 64; e++)
        {
            gr.ti[e] = (unsigned char) (e < npairs ? pair_i[e] : 0);
            gr.tj[e] = (unsigned char) (e < npairs ? pair_j[e] : 0);
        }
        if (use_vrows)
        {
            blocks = 0;
            // the wait below ends with the last kernel launched before it: this pass, or the last Gram riding behind it
            ride_enter = b->fprev && b->dl_n[0] >= 1 && gram_stash_feasible(c, b->dl_enter, b->dl_n[0]);
            ride_leave = b->fprev && b->dl_n[1] >= 1 && gram_stash_feasible(c, b->dl_leave, b->dl_n[1]);
            if (!ride_enter && !ride_leave)
                lbfgsx::poll_arm(c);
            if (col_a < 0)
                rc = launch_vrows_v<T>(c, tot, vsel_id, mask, pro, gr, nrows);
            else
                rc = launch_vrows<T, 20, 3>(c, tot, vsel_id, mask, pro, gr, nrows, col_a, col_b);
        }
        else if (ntot <= 11) blocks = launch_gram_vonly<T, 11>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
        else if (ntot <= 15) blocks = launch_gram_vonly<T, 15>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
        else if (ntot <= 23) blocks = launch_gram_vonly<T, 23>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
        else if (ntot <= 27) blocks = launch_gram_vonly<T, 27>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
        else blocks = launch_gram_vonly<T, 31>(c, nbatch, tot, vsel_id, mask, pro, gr, nrows);
    });
    if (compact_out)
        wf_rebuilt(c);
    if (kept)
    {
        b->wf_valid = true;  // usable by the passes of this subspace minimisation
        b->wf_epoch = b->sub_epoch;
        b->wf_ncorr = c->ncorr;
    }
    if (rc)
        return rc;
    if (blocks == 0)  // k_vrows: (hi, lo) of row r, entry j at gram_out[256 + 2 (r NP + j)]
    {
        // the carried first solve goes on to ask for the Grams over the rows that entered and left the free set
        // (lbfgsx_b_gram_list_dd): they ride behind this pass
        if (ride_enter)
            (void) gram_stash_launch(c, 1, 0, b->dl_enter, b->dl_n[0], /*signal=*/!ride_leave);
        if (ride_leave)
            (void) gram_stash_launch(c, 2, 0, b->dl_leave, b->dl_n[1], /*signal=*/true);
        double h[2 * 64];
        rc = fetch_gram_out(c, 256, 2 * 64, h);
        gram_stash_settle(c, rc == LBFGSX_OK);
        if (rc)
            return rc;
        for (int z = 0; z < npairs; z++)
        {
            out_dd[2 * z] = h[2 * slot[z]];
            out_dd[2 * z + 1] = h[2 * slot[z] + 1];
        }
        return LBFGSX_OK;
    }
    const int nch = std::min(blocks, 32);
    LBFGSX_LAUNCH(k_gram_finish, dim3(1, nch), dim3(kBlock), 0, c->stream, b->gram_partial, blocks, b->gram_partial2, 0);
    LBFGSX_LAUNCH(k_gram_finish, dim3(1, 1), dim3(kBlock), 0, c->stream, b->gram_partial2, nch, b->gram_out, 1, b->gram_dd);
    LBFGSX_HIP(hipGetLastError());
    if (b->gram_dd_host)
    {
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
        std::memcpy(out_dd, b->gram_dd_host, sizeof(double) * 2 * size_t(npairs));
        return LBFGSX_OK;
    }
    LBFGSX_HIP(lbfgsx::copy_async(out_dd, b->gram_dd, sizeof(double) * 2 * size_t(npairs), hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    return LBFGSX_OK;
}

// Gram of [Y_P S_P v_P] in ONE pass over the history; gram = 2c x 2c row-major, wtv = [Y'v, S'v] raw.
// k_gram_dd (correctly rounded double-double sums, 2c+1 <= 31), kx_gram beyond; LBFGSX_GRAM=i8 the exact integer-MFMA form.
// Returns LBFGSX_E_INVALID (outputs untouched) when none applies; the caller then falls back to lbfgsx_b_gram + lbfgsx_b_wtv.
int lbfgsx_b_gram_fused(lbfgsx_ctx* c, int mask, int vsel_id, double* gram, double* wtv)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    return lbfgsx_b_gram_fused_ex(c, mask, vsel_id, LBFGSX_GP_NONE, nullptr, nullptr, gram, wtv);
}

int lbfgsx_b_gram_fused_ex(lbfgsx_ctx* c, int mask, int vsel_id, int prologue, const double* coef1, const double* coef2,
                           double* gram, double* wtv)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    return lbfgsx_b_gram_fused_dd(c, mask, vsel_id, prologue, coef1, coef2, gram, wtv, nullptr);
}

int lbfgsx_b_gram_fused_dd(lbfgsx_ctx* c, int mask, int vsel_id, int prologue, const double* coef1, const double* coef2,
                           double* gram, double* wtv, double* gram_dd)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    return gram_dd_core(c, mask, vsel_id, prologue, coef1, coef2, gram, wtv, gram_dd, nullptr, 0);
}

int lbfgsx_b_gram_last_vrow_dd(lbfgsx_ctx* c, double* out_dd)
{
    if (!c || !c->bstate || !out_dd)
        return LBFGSX_E_INVALID;
    lbfgsb_state* b = c->bstate;
    if (!b->vrow_dd_valid)
    {
        set_error("lbfgsx_b_gram_last_vrow_dd: the last Gram pass left no un-rounded v row (no v, a list, or another pass since)");
        return LBFGSX_E_INVALID;
    }
    std::memcpy(out_dd, b->vrow_dd, sizeof(double) * size_t(4 * c->ncorr));
    return LBFGSX_OK;
}

}  // extern "C"
