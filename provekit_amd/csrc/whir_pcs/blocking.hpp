// blocking.hpp -- what the stand-alone entry points (pkw_evaluate, pkw_weighted_sums, pkw_sparse_*) share.  The argument rule, the
// segment sizes, the order of the steps and the copy out stay each entry's own.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/provekit_whir.h"

namespace pkw {

// one call's pk_malloc'ed device scratch, handed out front to back in field elements and freed when the call returns.  rc is
// pk_malloc's: nothing is taken unless it is PK_OK
struct Scratch {
    pk_ctx* const ctx;
    void* base = nullptr;
    const int rc;
    uint64_t* next;
    Scratch(pk_ctx* c, size_t fes) : ctx(c), rc(pk_malloc(c, 32 * fes, &base)), next((uint64_t*)base) {}
    Scratch(const Scratch&) = delete;
    ~Scratch() {
        if (!rc) pk_free(ctx, base);
    }
    uint64_t* take(size_t fes) {
        next += 4 * fes;
        return next - 4 * fes;
    }
};

// the operands are the context's work: finished before `launch` enqueues on the null stream, which is finished on return
template <class Launch>
int run_blocking(pk_ctx* ctx, Launch launch) {
    if (int rc = pk_ctx_sync(ctx)) return rc;
    if (int rc = launch()) return rc;
    return hipStreamSynchronize(nullptr) == hipSuccess ? PK_OK : PK_ERR_HIP;
}

}  // namespace pkw
