// conv_dgrad.h -- the summation order of the direct sparse-conv input gradient (conv_dgrad.hip), shared by the kernel's
// description and its host twin: every routine here is __host__ __device__, and the library is built with -ffp-contract=off.
//
//   dX[i][ci] = sum over offsets k, sum over channels co of dout[inv[k][i]][co] * W[k][ci][co]
//
// PINNED ORDER: an element of dX is ONE accumulator.  It starts at +0; the offsets k = 0 .. kvol - 1 are taken ascending, an
// offset whose entry inv[k][i] is no neighbour (dgrad_is_nbr) is skipped, and inside an offset the channels co = 0 .. cout - 1 are
// taken ascending, one dgrad_step -- one fused multiply-add, one rounding -- each.  The reduction is never split, so there are
// no segment boundaries: the value is a function of the row's neighbours, of the dout rows they name and of W alone.
// The kernel feeds the same chain to v_mfma_f32_32x32x2_f32, whose two reduction steps are two such fused steps in order.  It
// pads a row without the offset, a channel past cout and a column past cin with zeros: a step whose product is +-0 leaves an
// accumulator as it is, because a chain that starts at +0 never holds -0 (x + (-x) rounds to +0) short of underflow.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define DGRAD_HD __host__ __device__ __forceinline__

constexpr int kDgradMaxKvol = 27;

// an entry of the transposed rulebook is a neighbour iff it names one of the n_out rows of dout; any other value is never an address
DGRAD_HD bool dgrad_is_nbr(int v, int n_out) { return (unsigned)v < (unsigned)n_out; }

// one step of an element's chain: acc + g * w, rounded once (g = dout[inv[k][i]][co], w = W[k][ci][co])
DGRAD_HD float dgrad_step(float acc, float g, float w) { return fmaf(g, w, acc); }
