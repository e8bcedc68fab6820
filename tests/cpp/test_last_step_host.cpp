// tests/cpp/test_last_step_host.cpp -- the host rules of a deferred last recursion step (lbfgspp_amd/csrc/last_step.hpp),
// driven without a device: a vector stands in for the d buffer, "the step" adds one to it.  Built with
// -fsanitize=address,undefined by tests/test_last_step_host_cpu.py.  Prints "ok" and returns 0, or names the line that failed.
#include <cstdio>
#include <vector>

#include "../../lbfgspp_amd/csrc/last_step.hpp"

static int g_failed = 0;
#define EXPECT(cond)                                                  \
    do                                                                \
    {                                                                 \
        if (!(cond))                                                  \
        {                                                             \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            g_failed++;                                               \
        }                                                             \
    } while (0)

struct Buffers
{
    std::vector<double> d;  // the direction buffer: q before the step, d after it
    int steps_run = 0;
    int fail_next = 0;
    int last_num_slot = -1;  // which slot the step read the recursion's dot(0) from: 0 = its own, 1 = the keep slot
    int step(const lbfgsx::LastStep& ls)
    {
        if (fail_next)
        {
            fail_next = 0;
            return -3;
        }
        for (double& v : d)
            v += 1.0;
        steps_run++;
        last_num_slot = ls.taken ? 1 : 0;
        return 0;
    }
};

// a reader of d: settles first, then reads
static double read_d(lbfgsx::LastStep& ls, Buffers& b, int* rc = nullptr)
{
    const int r = ls.settle([&b](const lbfgsx::LastStep& s) { return b.step(s); });
    if (rc)
        *rc = r;
    return b.d[b.d.size() - 1];
}

int main()
{
    using lbfgsx::LastStep;
    // ---- when a product may end early
    {
        LastStep ls;
        EXPECT(ls.enabled);                                  // on by default
        EXPECT(!ls.want(true, true, true, 3, false, true));  // nobody asked
        ls.requested = true;
        EXPECT(ls.want(true, true, true, 3, false, true));
        EXPECT(!ls.want(false, true, true, 3, false, true));  // post form off
        EXPECT(!ls.want(true, false, true, 3, false, true));  // not a built-in objective
        EXPECT(!ls.want(true, true, false, 3, false, true));  // the search before did not accept its first trial
        EXPECT(!ls.want(true, true, true, 0, false, true));   // empty history
        EXPECT(!ls.want(true, true, true, 3, true, true));    // row shard
        EXPECT(!ls.want(true, true, true, 3, false, false));  // not the vector recursion
        ls.enabled = false;
        EXPECT(!ls.want(true, true, true, 3, false, true));  // switched off
    }
    // ---- nothing pending: a reader reads, no step runs
    {
        LastStep ls;
        Buffers b{std::vector<double>(5, 2.0)};
        EXPECT(read_d(ls, b) == 2.0 && b.steps_run == 0 && ls.settled == 0);
        EXPECT(!ls.fusable(true, true, true, 0));
    }
    // ---- deferred, then read: the step runs once, before the read
    {
        LastStep ls;
        Buffers b{std::vector<double>(5, 2.0)};
        ls.defer(3, 7, 1);
        EXPECT(ls.pending && !ls.taken && ls.cn == 3 && ls.col == 7 && ls.g == 1 && ls.deferred == 1);
        EXPECT(read_d(ls, b) == 3.0 && b.steps_run == 1 && b.last_num_slot == 0);
        EXPECT(!ls.pending && ls.settled == 1);
        EXPECT(read_d(ls, b) == 3.0 && b.steps_run == 1);  // a second reader finds d
    }
    // ---- which trial may run the step
    {
        LastStep ls;
        ls.defer(2, 4, 1);
        EXPECT(ls.fusable(true, true, true, 1));
        EXPECT(!ls.fusable(false, true, true, 1));  // not the post-form first trial
        EXPECT(!ls.fusable(true, false, true, 1));  // not a built-in objective
        EXPECT(!ls.fusable(true, true, false, 1));  // the caller does not read grad.d from it
        EXPECT(!ls.fusable(true, true, true, 2));   // the search starts from another point
    }
    // ---- fused and accepted: d is never formed; the next product drops the debt
    {
        LastStep ls;
        Buffers b{std::vector<double>(5, 2.0)};
        ls.defer(2, 4, 1);
        ls.owe();
        EXPECT(ls.owed);
        ls.fuse();
        EXPECT(ls.pay() && !ls.owed && !ls.pay());
        EXPECT(ls.pending && ls.taken && ls.fused == 1);
        EXPECT(!ls.fusable(true, true, true, 1));  // not twice
        ls.drop();
        EXPECT(!ls.pending && !ls.taken && b.steps_run == 0);
        EXPECT(read_d(ls, b) == 2.0 && b.steps_run == 0);
    }
    // ---- fused and rejected: the second trial settles, reading dot(0) from its keep slot
    {
        LastStep ls;
        Buffers b{std::vector<double>(5, 2.0)};
        ls.defer(2, 4, 1);
        ls.fuse();
        EXPECT(read_d(ls, b) == 3.0 && b.steps_run == 1 && b.last_num_slot == 1);
        EXPECT(!ls.pending && !ls.taken && ls.settled == 1 && ls.fused == 1);
    }
    // ---- a download between the product and the search: the step settles, grad.d is still owed to the first trial
    {
        LastStep ls;
        Buffers b{std::vector<double>(5, 2.0)};
        ls.defer(2, 4, 1);
        ls.owe();
        EXPECT(read_d(ls, b) == 3.0);
        EXPECT(!ls.fusable(true, true, true, 1) && ls.owed && ls.cn == 2);
        EXPECT(ls.pay() && !ls.pay());
    }
    // ---- a step launch that fails leaves the step pending and is reported
    {
        LastStep ls;
        Buffers b{std::vector<double>(5, 2.0)};
        ls.defer(1, 0, 0);
        b.fail_next = 1;
        int rc = 0;
        (void) read_d(ls, b, &rc);
        EXPECT(rc == -3 && ls.pending && ls.settled == 0 && b.steps_run == 0);
        EXPECT(read_d(ls, b, &rc) == 3.0 && rc == 0 && !ls.pending && ls.settled == 1);
    }
    // ---- owe() without a pending step owes nothing; a new deferral starts clean
    {
        LastStep ls;
        ls.owe();
        EXPECT(!ls.owed);
        ls.defer(2, 1, 0);
        ls.fuse();
        ls.defer(3, 2, 1);
        EXPECT(ls.pending && !ls.taken && ls.deferred == 2);
    }
    if (g_failed)
        return 1;
    std::printf("ok\n");
    return 0;
}
