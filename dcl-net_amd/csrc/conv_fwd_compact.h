// conv_fwd_compact.h -- the summation order of the compact sparse-conv forward (conv_fwd_compact.hip), shared by the kernel's
// description and its host twin: every routine here is __host__ __device__, and the library is built with -ffp-contract=off.
//
//   out[o][co] = sum over offsets k, sum over channels ci of X[nbr[k][o]][ci] * W[k][ci][co]
//
// PINNED ORDER: an element of out is an accumulator acc that starts at +0.  The offsets are visited in the forward's visiting
// order (cfc_offset_at: k ascending, the centre first for subm -- conv_body.h: offset_at); an offset whose entry nbr[k][o] is no
// neighbour (cfc_is_nbr) is skipped.  A visited offset forms ITS OWN chain, part, from +0 over the channels ci = 0 .. cin - 1
// ascending, one cfc_step -- one fused multiply-add, one rounding -- each, and is then added with ONE fp32 add (cfc_add):
// the reference's own association (a GEMM per offset, then a scatter-add) and the order conv_stem_body uses.  A row without
// neighbours is +0.  The value is a function of the row's neighbours, of the X rows they name and of W alone.
// The kernel feeds part's chain to v_mfma_f32_32x32x2_f32, whose two reduction steps are two such fused steps in order, with
// accumulators that start at zero for every block of pairs.  It pads a channel past cin and a column past cout with zeros: a
// step whose product is +-0 leaves a chain as it is, because a chain that starts at +0 never holds -0 (x + (-x) rounds to
// +0) short of underflow.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define CFC_HD __host__ __device__ __forceinline__

constexpr int kCfcMaxKvol = 27;

// an entry of the rulebook is a neighbour iff it names one of the n_in rows of X; any other value is never an address
CFC_HD bool cfc_is_nbr(int v, int n_in) { return (unsigned)v < (unsigned)n_in; }

// the offset visited at `step`: the centre first for subm, the others ascending
CFC_HD int cfc_offset_at(int step, int kvol, int subm) {
  if (!subm) return step;
  const int centre = kvol / 2;
  if (step == 0) return centre;
  return step <= centre ? step - 1 : step;
}

// one step of an offset's chain: part + x * w, rounded once (x = X[nbr[k][o]][ci], w = W[k][ci][co])
CFC_HD float cfc_step(float part, float x, float w) { return fmaf(x, w, part); }

// a finished offset joins the element: one fp32 add
CFC_HD float cfc_add(float acc, float part) { return acc + part; }
