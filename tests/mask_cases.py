"""The masks the mask-to-box tests run on -- the smallest ones on which a run-labelling kernel goes wrong -- and an independent
restatement of ops.mask_box's semantics (scipy.ndimage.label with a 3 x 3 structure + find_objects + the selection and tie
rule + crops.lm_box + the clamp) that the host twin is compared with."""
import numpy as np

SIZES = [(480, 640), (37, 70)]          # the loaders' frame; no multiple of 32 and narrower than three words


def _ring(H, W, thick):
    m = np.zeros((H, W), bool)
    r0, r1, c0, c1 = H // 5, H - H // 5, W // 6, W - W // 6
    m[r0:r1, c0:c1] = True
    m[r0 + thick:r1 - thick, c0 + thick:c1 - thick] = False
    return m


def _spiral(H, W):
    """a rectangular spiral of one-pixel arms, two pixels apart: labels of far-apart rows meet late"""
    m = np.zeros((H, W), bool)
    t, b, l, r = 1, H - 2, 1, W - 2
    first = True
    while b - t >= 2 and r - l >= 2:
        m[t, (l if first else l - 2):r + 1] = True           # the top arm reaches back to the left arm of the turn before
        m[t:b + 1, r] = True
        m[b, l:r + 1] = True
        m[t + 2:b + 1, l] = True
        t, b, l, r = t + 2, b - 2, l + 2, r - 2
        first = False
    return m


def mask_cases(H, W):
    """-> list of (name, (H,W) bool mask)"""
    out = []
    z = lambda: np.zeros((H, W), bool)
    out.append(("empty", z()))
    out.append(("full", np.ones((H, W), bool)))
    m = z(); m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = True
    out.append(("corners", m))
    m = z(); m[5:12, 6:14] = True; m[12:20, 14:30] = True                      # touch at one corner only
    out.append(("diagonal touch", m))
    m = z(); m[5:12, 6:14] = True; m[13:20, 6:30] = True; m[5:12, 15:19] = True   # one clear row / column between them
    out.append(("one pixel apart", m))
    m = z(); m[3, 20:32] = True; m[4, 32:40] = True; m[8, 0:32] = True; m[9, 33:64] = True
    out.append(("word boundary", m))
    out.append(("ring", _ring(H, W, 4)))
    out.append(("thin ring", _ring(H, W, 1)))
    m = z(); m[4:H - 4, 5] = True; m[4:H - 4, W - 6] = True; m[H - 5, 5:W - 5] = True
    out.append(("U", m))
    out.append(("spiral", _spiral(H, W)))
    m = z(); m[2:H - 2, 3:W - 3:2] = True; m[H - 3, 3:W - 3] = True
    out.append(("comb", m))
    yy, xx = np.mgrid[0:H, 0:W]
    out.append(("checkerboard", (yy + xx) % 2 == 0))
    m = z(); m[:, 0::2] = True
    out.append(("stripes", m))
    for p in (0.2, 0.41, 0.6):
        for seed in (1, 2, 3):
            out.append(("bernoulli %.2f seed %d" % (p, seed), np.random.default_rng(seed).random((H, W)) < p))
    m = z(); m[3:9, 4:14] = True; m[20:30, 40:46] = True; m[15:17, 20:22] = True    # 6 x 10 and 10 x 6: equal areas
    out.append(("tie", m))
    return out


def winner(mask):
    """((x, y, w, h, pixel count) of the winning component or None, number of components) from scipy's labelling"""
    from scipy import ndimage
    H, W = mask.shape
    lab, ncomp = ndimage.label(mask, structure=np.ones((3, 3), int))
    if ncomp == 0:
        return None, 0
    ids = np.arange(1, ncomp + 1)
    first = ndimage.minimum(np.arange(H * W).reshape(H, W), lab, ids)          # raster index of every component's first pixel
    npix = np.bincount(lab.ravel(), minlength=ncomp + 1)[1:]
    best, best_key = None, (0, -1)
    for k, sl in enumerate(ndimage.find_objects(lab)):
        y0, y1, x0, x1 = sl[0].start, sl[0].stop, sl[1].start, sl[1].stop
        key = ((x1 - x0) * (y1 - y0), int(first[k]))      # largest rectangle; among equal ones the LAST first pixel
        if key > best_key:
            best_key, best = key, (x0, y0, x1 - x0, y1 - y0, int(npix[k]))
    return best, ncomp


def restate(mask, padding, lm_box, won=None):
    """the ten integers of ops.mask_box for one (H,W) bool mask (won: winner(mask), to share it among paddings)"""
    H, W = mask.shape
    best, ncomp = winner(mask) if won is None else won
    if best is None:
        box, npix = [0, 0, 0, 0], 0
    else:
        box, npix = [best[0] - padding // 2, best[1] - padding // 2, best[2] + padding, best[3] + padding], best[4]
    r0, r1, c0, c1 = lm_box(box, H, W)
    return np.array(box + [max(r0, 0), min(r1, H), max(c0, 0), min(c1, W), ncomp, npix], np.int32)
