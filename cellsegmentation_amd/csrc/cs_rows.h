// Row passes over NHWC rows [M][C]: the one thread placement of the BatchNorm passes (bn.hip) and the per-sample row sums (dwse.hip).  Device code plus the small host struct, like cs_block.h.
//
// Layout contract.  A launch is (row blocks) x (channel chunks of <= cw 8-channel groups).  Inside a 256-thread workgroup
//     tid = rr * width + cgl          cgl < width: the thread's 8-channel group inside the chunk, cg = cg0 + cgl in the tensor
//                                     rr: its row lane; lanes rr < rpar = 256 / width are LIVE, the 256 - rpar * width others idle
// where width = min(cw, CG - cg0) is the chunk's own width (the last chunk may be narrower).  A live thread keeps ONE channel group, so
// every per-channel constant is loaded once per thread, and walks rows r0 + rr, r0 + rr + rpar, ... < r1 of its workgroup's row block
// [r0, r1) = [block * rows_per_block, min(M, (block + 1) * rows_per_block)).  The LDS folds that follow a reduction index their partials
// by tid, i.e. fold[rr * width + cgl], and add lanes rr = 0 .. rpar - 1 in ascending order.
#pragma once
#include "cs_common.h"

// host: what a launch rule decides -- channel chunks, 8-channel groups per chunk, rows per workgroup
struct RowSplit {
    int chunks, cw, rpb;
    long long row_blocks(long long M) const { return (M + rpb - 1) / rpb; }
    dim3 grid(long long M) const { return dim3((unsigned)row_blocks(M), (unsigned)chunks); }      // (row blocks, channel chunks)
};

// Row: the row index type (long long for tensors of M rows, int for the rows of one sample)
template <typename Row = long long>
struct RowLane {
    int cg0, width, rpar, cgl, cg, rr;
    bool live;
    Row r0, r1;
    __device__ __forceinline__ RowLane(unsigned row_block, unsigned chunk, int cw, int CG, int rows_per_block, Row M) {
        cg0 = (int)chunk * cw;
        width = (CG - cg0) < cw ? (CG - cg0) : cw;
        rpar = 256 / width;
        cgl = (int)(threadIdx.x % width);
        cg = cg0 + cgl;
        rr = threadIdx.x / width;
        live = rr < rpar;
        r0 = (Row)row_block * rows_per_block;
        r1 = r0 + rows_per_block;
        if (r1 > M) r1 = M;
    }
};

// The walk itself stays written out in each kernel (first row r0 + rr, steps of U * rpar with U rows in flight, single rows after):
// a walker that hands the rows to one generic body was tried and gave other bits and other speed.  Several bodies hold `a * b + c`
// chains (the SiLU derivative of the BatchNorm backward, the fp32 product sum v0 * w0 + v1 * w1 of sample_rowsum_kernel) that the
// compiler contracts into fused multiply-adds for some of a thread's eight channels and not for others, and which ones follows the
// exact form of the loop -- and with it the last bit of the result; bn_apply_kernel came out 1.2 % slower.
// tests/test_row_passes_bits_gpu.py holds every row pass to its recorded bits.
