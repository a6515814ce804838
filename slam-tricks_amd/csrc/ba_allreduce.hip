// ba_allreduce.hip -- the cross-rank sum of the reduced system of a sharded bundle adjustment (CrossRankSum, ba_engine.hpp): the two
// pack kernels, the plan of what travels, and the pack / hook / unpack sequence that ba_build_reduced (ba_linear.hip) calls as one
// step.  The trial block's five summed scalars go through the same hook in ba_trial.
#include <vector>

#include "ba_engine.hpp"

namespace stba {

// row r < n: S[r][0..r] <-> tri[r(r+1)/2 ..]; block n: the four extras vectors behind S <-> behind tri
__global__ __launch_bounds__(256) void tri_pack_kernel(double* __restrict__ Sbuf, int lda, int n, double* __restrict__ pack, int to_pack) {
    const int r = blockIdx.x;
    if (r < n) {
        double* row = Sbuf + (size_t)r * lda;
        double* dst = pack + (size_t)r * (r + 1) / 2;
        for (int c = threadIdx.x; c <= r; c += 256) {
            if (to_pack) dst[c] = row[c]; else row[c] = dst[c];
        }
    } else {
        double* ex = Sbuf + (size_t)lda * lda;
        double* dst = pack + (size_t)n * (n + 1) / 2;
        for (int c = threadIdx.x; c < 4 * lda; c += 256) {
            if (to_pack) dst[c] = ex[c]; else ex[c] = dst[c];
        }
    }
}

// the travelling 6x6 blocks <-> the packed buffer; the four extras vectors behind S <-> behind the blocks
__global__ __launch_bounds__(256) void blk_pack_kernel(double* __restrict__ Sbuf, int lda, const int2* __restrict__ blocks, int nz,
                                                       double* __restrict__ pack, int to_pack) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nel = (size_t)nz * 36;
    if (e < nel) {
        const int blk = (int)(e / 36), k = (int)(e % 36);
        const int2 ij = blocks[blk];
        double* p = Sbuf + (size_t)(6 * ij.x + k / 6) * lda + 6 * ij.y + k % 6;
        if (to_pack) pack[e] = *p; else *p = pack[e];
    } else if (e < nel + 4 * (size_t)lda) {
        double* p = Sbuf + (size_t)lda * lda + (e - nel);
        if (to_pack) pack[e] = *p; else *p = pack[e];
    }
}

// decides once per engine what travels in the cross-rank sum of the reduced system: the union over ranks of the
// non-zero blocks (a 0/1 mask of the nc(nc+1)/2 lower blocks, summed with the same hook) if it is sparse
static int ba_plan_pack(stba_ba* b) {
    const size_t nb = (size_t)b->nc * (b->nc + 1) / 2;
    static const bool SPARSE = knob_int("STBA_PACK_BLOCKS", 1) != 0;
    b->ar.form = PACK_TRIANGLE;
    if (SPARSE && !b->ar.h_row_col_ptr.empty()) {
        std::vector<double> mask(nb, 0.0);
        for (int c = 0; c < b->nc; ++c) {
            mask[(size_t)c * (c + 1) / 2 + c] = 1.0;                 // the diagonal block always travels (Hcc)
            for (int k = b->ar.h_row_col_ptr[(size_t)c]; k < b->ar.h_row_col_ptr[(size_t)c + 1]; ++k)
                mask[(size_t)c * (c + 1) / 2 + b->ar.h_row_cols[(size_t)k]] = 1.0;
        }
        DevBuf<double> dmask;
        STBA_TRY(dmask.alloc(nb));
        STBA_TRY(upload(dmask, mask.data(), nb, b->st));
        if (b->ar.fn(b->ar.user, dmask, nb, b->st) != 0) return fail(STBA_ERR_CALLBACK, "all-reduce hook failed");
        if (hipMemcpyAsync(mask.data(), dmask, nb * sizeof(double), hipMemcpyDeviceToHost, b->st) != hipSuccess ||
            hipStreamSynchronize(b->st) != hipSuccess)
            return fail(STBA_ERR_HIP, "mask download failed");
        dmask.reset();
        std::vector<int2> blocks;
        for (int c = 0; c < b->nc; ++c)
            for (int c2 = 0; c2 <= c; ++c2)
                if (mask[(size_t)c * (c + 1) / 2 + c2] > 0.5) blocks.push_back(make_int2(c, c2));
        if (blocks.size() * 36 * 2 < (size_t)b->n * (b->n + 1) / 2) {      // worth it below 50 % of the triangle
            STBA_TRY(b->ar.blocks.alloc(blocks.size()));
            STBA_TRY(upload(b->ar.blocks, blocks.data(), blocks.size(), b->st));
            STBA_HIP(hipStreamSynchronize(b->st));
            b->ar.nz = (int)blocks.size();
            b->ar.form = PACK_BLOCKS;
        }
    }
    STBA_TRY(b->ar.Spack.alloc(b->ar.pack_count(b->n, b->lda)));
    return STBA_OK;
}

// device time of the last cross-rank sum of the reduced system: read once its events have completed (after a
// synchronisation of the stream; a pair still in flight is waited for -- only on the multi-rank path)
void ba_collect_allreduce_time(stba_ba* b) {
    if (!b->ar.timing_pending) return;
    float ms = 0.f;
    if (hipEventSynchronize(b->ar.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, b->ar.ev[0], b->ar.ev[1]) == hipSuccess) b->ar.ms += ms;
    b->ar.timing_pending = false;
}

// the reduced system of this rank -> the sum over ranks, in place: pack the lower triangle + extras (half the bytes on the wire: 144 MB
// instead of 288 MB at C5) or the travelling blocks + extras, sum across ranks, unpack
int ba_allreduce_system(stba_ba* b) {
    if (b->ar.form == PACK_UNPLANNED) STBA_TRY(ba_plan_pack(b));
    const unsigned pgrid = (unsigned)((b->ar.pack_count(b->n, b->lda) + 255) / 256);
    if (b->ar.form == PACK_BLOCKS) hipLaunchKernelGGL(blk_pack_kernel, dim3(pgrid), dim3(256), 0, b->st, b->Sbuf, b->lda, b->ar.blocks, b->ar.nz, b->ar.Spack, 1);
    else hipLaunchKernelGGL(tri_pack_kernel, dim3(b->n + 1), dim3(256), 0, b->st, b->Sbuf, b->lda, b->n, b->ar.Spack, 1);
    ba_collect_allreduce_time(b);                     // (a previous build's pair, if nobody has read it yet)
    if (b->ar.timing_on) {
        if (!b->ar.ev[0]) { STBA_TRY(b->ar.ev[0].create()); STBA_TRY(b->ar.ev[1].create()); }
        STBA_HIP(hipEventRecord(b->ar.ev[0], b->st));
    }
    if (b->ar.fn(b->ar.user, b->ar.Spack, b->ar.pack_count(b->n, b->lda), b->st) != 0)
        return fail(STBA_ERR_CALLBACK, "all-reduce hook failed");
    if (b->ar.timing_on) { STBA_HIP(hipEventRecord(b->ar.ev[1], b->st)); b->ar.timing_pending = true; }
    b->ar.bytes += (double)b->ar.pack_count(b->n, b->lda) * sizeof(double);
    b->ar.calls += 1;
    if (b->ar.form == PACK_BLOCKS) hipLaunchKernelGGL(blk_pack_kernel, dim3(pgrid), dim3(256), 0, b->st, b->Sbuf, b->lda, b->ar.blocks, b->ar.nz, b->ar.Spack, 0);
    else hipLaunchKernelGGL(tri_pack_kernel, dim3(b->n + 1), dim3(256), 0, b->st, b->Sbuf, b->lda, b->n, b->ar.Spack, 0);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

}  // namespace stba
