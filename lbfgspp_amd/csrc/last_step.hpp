// lbfgspp_amd/csrc/last_step.hpp -- host state of a two-loop product whose last step is still to run.
//
// A persistent launch from the gradient may end with step 2c-1 (PersistArgs::defer_last, lbfgs_kernels.cuh).  The d buffer
// then holds q before the last update, and one of two passes runs step 2c:
//   * the first trial of the next search, in the last form (k_trial_last): it forms d in registers and does not store it.
//     If the search accepts that trial, d is never read and the next product overwrites the buffer;
//   * a k_twoloop<TL_ADD> launch ("settling"), the same statement with the same bits, ahead of ANY other reader of d: a
//     download, a getter, a plain trial, the second trial of a search whose first one was rejected.
// The rules live here, free of device code, so that a host program can drive them (tests/cpp/test_last_step_host.cpp).
#pragma once
#include <cstdint>

namespace lbfgsx {

struct LastStep
{
    bool enabled = true;     // LBFGSX_LAST_IN_TRIAL=0: never defer (read once, at creation)
    bool requested = false;  // the driver takes grad.d from its first trial (lbfgsx_last_in_trial_request)
    bool pending = false;    // the d buffer holds q before the last update
    bool taken = false;      // a last-form trial ran the step: the recursion's dot(0) has moved to its keep slot
    int cn = 0;              // pairs of the product
    int col = 0;             // physical column of its newest pair
    int g = 0;               // buffer of the gradient it was computed from
    bool owed = false;       // the caller was told "pending" in place of grad.d: its first trial returns it, however the step ran
    int64_t deferred = 0, fused = 0, settled = 0;  // instrumentation (lbfgsx_last_in_trial_counts)

    // May the product that follows an accepted post-form first trial end one step early?  Only where the next search's first
    // trial will be a post-form one as far as the context can tell, and only for a caller that can do without grad.d.
    bool want(bool post_form_on, bool builtin_objective, bool first_trial_accepted, int pairs, bool sharded,
              bool vector_recursion) const
    {
        return enabled && requested && post_form_on && builtin_objective && first_trial_accepted && pairs >= 1 && !sharded &&
               vector_recursion;
    }
    // the persistent launch ran to its end with defer_last
    void defer(int pairs, int newest_col, int g_buf)
    {
        pending = true;
        taken = owed = false;
        cn = pairs;
        col = newest_col;
        g = g_buf;
        deferred++;
    }
    // May this trial run the step?  The first trial of a search, in the post form, of a built-in objective, by a caller that
    // reads grad.d from it, from the point whose gradient the product used.
    bool fusable(bool post_form, bool builtin_objective, bool caller_reads_dg, int xp_buf) const
    {
        return pending && !taken && post_form && builtin_objective && caller_reads_dg && xp_buf == g;
    }
    void fuse()
    {
        taken = true;
        fused++;
    }
    // Any other reader of d: run the step first.  launch(const LastStep&) enqueues k_twoloop<TL_ADD> and returns 0 or an error,
    // which leaves the step pending.
    template <class F>
    int settle(F&& launch)
    {
        if (!pending)
            return 0;
        const int rc = launch(static_cast<const LastStep&>(*this));
        if (rc)
            return rc;
        pending = taken = false;
        settled++;
        return 0;
    }
    // the product's caller gets "pending" in place of grad.d
    void owe() { owed = pending; }
    // a trial that returns grad.d to its caller: true when that caller is still waiting for it
    bool pay()
    {
        const bool was = owed;
        owed = false;
        return was;
    }
    // the d buffer is about to be overwritten (the next product, a reset): nothing is owed any more
    void drop() { pending = taken = owed = false; }
};

}  // namespace lbfgsx
