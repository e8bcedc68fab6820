// lbfgspp_amd/csrc/dense_topology.hip -- the matrix of a dense linear-model objective on the context (include/lbfgsx.h,
// "dense linear-model objectives"; walked by linear_dense_kernels.cuh).  It holds no kernel: the form's seven are compiled
// with the caller's text (jit_objective.hip), k_dense_partials among them.
//
//   a HOST matrix (R x F, row stride lda) is copied into an array the context owns, compactly (row stride F);
//   a DEVICE matrix is used in place: no copy is made -- duplicating it is what would make dense data infeasible -- and the
//   caller keeps it alive and unchanged while the objective is bound.
// Either way the context allocates w[R*D], v[R] and part[chunks*n], chunks = ceil(R / C), C = kDenseChunk.  The arguments
// were validated by lbfgsx_objective_bind_dense.
#include "launch_args.hpp"

namespace lbfgsx {

void dense_topology_free(lbfgsx_ctx* c)
{
    lbfgsx_ctx::DenseTopo& d = c->dense;
    if (d.own)
        (void) hipFree(const_cast<void*>(d.A));
    (void) hipFree(d.w);
    (void) hipFree(d.v);
    (void) hipFree(d.part);
    d = lbfgsx_ctx::DenseTopo();
}

namespace {

int build(lbfgsx_ctx* c, int64_t R, int D, const void* A, int64_t lda, int on_device, int lanes)
{
    lbfgsx_ctx::DenseTopo& d = c->dense;
    const size_t esz = size_t(c->esz);
    const int64_t F = c->n / D;
    d.R = R;
    d.F = F;
    d.D = D;
    d.C = kDenseChunk;
    d.chunks = (R + kDenseChunk - 1) / kDenseChunk;
    d.L = lanes ? lanes : linear_lanes_rule(1, F);
    if (on_device)
    {
        d.A = A;
        d.lda = lda;
        d.own = false;
    }
    else
    {
        void* copy = nullptr;
        LBFGSX_HIP(hipMalloc(&copy, size_t(R) * size_t(F) * esz));
        d.A = copy;
        d.lda = F;
        d.own = true;
        LBFGSX_HIP(hipMemcpy2DAsync(copy, size_t(F) * esz, A, size_t(lda) * esz, size_t(F) * esz, size_t(R), hipMemcpyHostToDevice,
                                    c->stream));
    }
    LBFGSX_HIP(hipMalloc(&d.w, size_t(R) * size_t(D) * esz));
    LBFGSX_HIP(hipMalloc(&d.v, size_t(R) * esz));
    LBFGSX_HIP(hipMalloc(&d.part, size_t(d.chunks) * size_t(c->n) * esz));
    LBFGSX_HIP(stream_sync(c->stream));  // the caller's host matrix may go when this returns
    return LBFGSX_OK;
}

}  // namespace

int dense_topology_build(lbfgsx_ctx* c, int64_t R, int D, const void* A, int64_t lda, int on_device, int lanes)
{
    LBFGSX_HIP(stream_sync(c->stream));  // no launch of an earlier binding still reads what this call frees
    graph_topology_free(c);
    const int rc = build(c, R, D, A, lda, on_device, lanes);
    if (rc)
    {
        (void) stream_sync(c->stream);
        dense_topology_free(c);
    }
    return rc;
}

int dense_topology_read(lbfgsx_ctx* c, void* w, void* v, void* part)
{
    const lbfgsx_ctx::DenseTopo& d = c->dense;
    const size_t esz = size_t(c->esz);
    if (w)
        LBFGSX_HIP(copy_async(w, d.w, size_t(d.R) * size_t(d.D) * esz, hipMemcpyDeviceToHost, c->stream));
    if (v)
        LBFGSX_HIP(copy_async(v, d.v, size_t(d.R) * esz, hipMemcpyDeviceToHost, c->stream));
    if (part)
        LBFGSX_HIP(copy_async(part, d.part, size_t(d.chunks) * size_t(c->n) * esz, hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(stream_sync(c->stream));
    return LBFGSX_OK;
}

}  // namespace lbfgsx
