// mask_box.h -- what the device kernels (mask_box.hip) and their host twin (dcl_mask_box_host) share of the loaders'
// `get_bbox(mask_to_bbox(mask_label, padding))` (LM/dataloader_test_LMO.py:26-42,360-402; LM/dataloader_test_LM.py:16,144):
// which connected piece of the mask wins, and the integer arithmetic from the winner's rectangle to the crop rows.
//
// Semantics (n label images per call, int32 (n,H,W)):
//   set pixel      label == value
//   component      an 8-connected set of set pixels; pixels on the image border count like any others
//   rectangle      x = min col, y = min row, w = max col - min col + 1, h = max row - min row + 1 (cv2.boundingRect)
//   winner         the component with the largest w * h (hole contours cannot change it: their rectangles lie inside their
//                  component's); among equal areas the one whose first pixel in raster order comes LAST (mb_better below)
//   box            [x - padding / 2, y - padding / 2, w + padding, h + padding]; [0, 0, 0, 0] when no pixel is set
//   crop           crops.lm_box(box, H, W) -> (r0, r1, c0, c1), then max(r0, 0), min(r1, H), max(c0, 0), min(c1, W): the
//                  row CropBuilder.build_lm hands to dcl_crop_points
//   out[10]        box[4], crop[4], number of components, pixel count of the winner
//
// TWO ASSUMPTIONS ARE NOT PINNED AGAINST cv2 (it is not installed where this project is built and tested):
//   * the tie rule.  The reference keeps the first strict maximum in cv2.findContours' order; OpenCV hands contours out in
//     reverse order of discovery, hence "the component found last in a raster scan wins a tie".  It lives in mb_better and
//     nowhere else.
//   * the border rule.  Older OpenCV releases clear the outermost pixel ring of the image before tracing contours; here a
//     border pixel is a pixel.
// Neither matters for a mask whose largest rectangle is unique and does not rest on the image border alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MB_HD __host__ __device__ inline
#else
#define MB_HD inline
#endif

// a component: its rectangle's area, the raster index (row * W + col) of its first pixel, its rectangle and pixel count
struct MbComp {
  long long area, first;
  int x0, x1, y0, y1, npix;
};

MB_HD MbComp mb_none() { return MbComp{0, -1, 0, 0, 0, 0, 0}; }

// THE tie rule: does component a beat component b?  Larger rectangle; among equal ones the later first pixel.
MB_HD bool mb_better(const MbComp &a, const MbComp &b) { return a.area > b.area || (a.area == b.area && a.first > b.first); }

// first_col: the column of the component's first pixel in raster order (it lies in row y0, the component's top row)
MB_HD MbComp mb_comp(int x0, int x1, int y0, int y1, int npix, int first_col, int W) {
  return MbComp{(long long)(x1 - x0 + 1) * (y1 - y0 + 1), (long long)y0 * W + first_col, x0, x1, y0, y1, npix};
}

// one side of `get_bbox`: lengths strictly between two borders of -1, 40, 80 ... 680 grow to the upper one (0 -> 40)
MB_HD int mb_grow(int v) { return (v > -1 && v < 680 && (v % 40 != 0 || v == 0)) ? (v / 40 + 1) * 40 : v; }

// crops.lm_box: [x, y, w, h] -> (rmin, rmax, cmin, cmax); every quantity that is halved is >= 0 for the boxes made here
MB_HD void mb_lm_box(const int *bb, int H, int W, int *out) {
  int r0 = bb[1], r1 = bb[1] + bb[3], c0 = bb[0], c1 = bb[0] + bb[2];
  r0 = r0 < 0 ? 0 : r0;
  c0 = c0 < 0 ? 0 : c0;
  r1 = r1 >= H ? H - 1 : r1;
  c1 = c1 >= W ? W - 1 : c1;
  const int hr = mb_grow(r1 - r0) / 2, hc = mb_grow(c1 - c0) / 2;
  const int mr = (r0 + r1) / 2, mc = (c0 + c1) / 2;
  r0 = mr - hr; r1 = mr + hr; c0 = mc - hc; c1 = mc + hc;
  if (r0 < 0) { r1 -= r0; r0 = 0; }
  if (c0 < 0) { c1 -= c0; c0 = 0; }
  if (r1 > H) { r0 -= r1 - H; r1 = H; }
  if (c1 > W) { c0 -= c1 - W; c1 = W; }
  out[0] = r0; out[1] = r1; out[2] = c0; out[3] = c1;
}

// winner (ncomp == 0: none) -> the ten output integers
MB_HD void mb_finish(const MbComp &win, int ncomp, int padding, int H, int W, int32_t *out) {
  int bb[4] = {0, 0, 0, 0};
  if (ncomp > 0) {
    bb[0] = win.x0 - padding / 2; bb[1] = win.y0 - padding / 2;
    bb[2] = win.x1 - win.x0 + 1 + padding; bb[3] = win.y1 - win.y0 + 1 + padding;
  }
  int c[4];
  mb_lm_box(bb, H, W, c);
  out[0] = bb[0]; out[1] = bb[1]; out[2] = bb[2]; out[3] = bb[3];
  out[4] = c[0] < 0 ? 0 : c[0]; out[5] = c[1] > H ? H : c[1];
  out[6] = c[2] < 0 ? 0 : c[2]; out[7] = c[3] > W ? W : c[3];
  out[8] = ncomp; out[9] = ncomp > 0 ? win.npix : 0;
}

// sizes: 32-bit words per row, and the most runs a mask can hold (every other pixel of every row)
MB_HD int mb_words_per_row(int W) { return (W + 31) / 32; }
MB_HD long long mb_run_cap(int H, int W) { return (long long)H * ((W + 1) / 2); }
