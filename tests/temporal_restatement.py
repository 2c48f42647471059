"""Temporal accumulation by reprojection, restated in numpy float32 from the text of include/pt_hip.h (pt_temporal_push_host) --
not from the kernel.  Every operation below is one correctly rounded float operation in the order the header states, so the
device must reproduce these arrays bit for bit.

    camera_inverse   rows i0, i1, i2 of the inverse of [right up forward], in double, rounded to float once
    Temporal         the state of one view sequence; push() takes a frame's accumulators, its feature dict (as
                     denoise_restatement.features returns it) and its camera (4 x 3: origin, right, up, forward)
"""
import numpy as np

import view_composition as V

F32 = np.float32
DEFAULT_MAX_FRAMES = F32(32.0)
DEFAULT_SIGMA_PLANE = F32(0.1)
DEFAULT_MIN_NORMAL_DOT = F32(0.9)
MIN_WEIGHT = F32(1e-3)


def camera_inverse(camera):
    cam = np.asarray(camera, np.float32).reshape(4, 3).astype(np.float64)
    r, u, f = cam[1], cam[2], cam[3]

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float64)

    c = cross(u, f)
    det = (r[0] * c[0] + r[1] * c[1]) + r[2] * c[2]
    return np.stack([cross(u, f) / det, cross(f, r) / det, cross(r, u) / det]).astype(np.float32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class Temporal:
    """State after a push: H [H, W, 8] = Hs[3], Hn, Hs2[3], HL; the frame's P', N', class and camera."""

    def __init__(self, width, height):
        self.W, self.H = width, height
        self.reset()

    def reset(self):
        self.Hrec = None

    def push(self, s, s2, c, feat, camera=None, max_frames=0.0, sigma_plane=0.0, min_normal_dot=0.0):
        """dict of sum, sum2 [n, 3], count [n] (int32), history_frames [n]."""
        W, H = self.W, self.H
        max_frames = F32(max_frames) if max_frames > 0 else DEFAULT_MAX_FRAMES
        sigma_plane = F32(sigma_plane) if sigma_plane > 0 else DEFAULT_SIGMA_PLANE
        min_normal_dot = F32(min_normal_dot) if min_normal_dot > 0 else DEFAULT_MIN_NORMAL_DOT
        cam = np.asarray(V.REFERENCE_CAMERA if camera is None else camera, np.float32).reshape(4, 3).copy()
        s = np.ascontiguousarray(s, np.float32).reshape(H, W, 3)
        s2 = np.ascontiguousarray(s2, np.float32).reshape(H, W, 3)
        c = np.ascontiguousarray(c, np.int32).reshape(H, W)
        P = np.ascontiguousarray(feat["position"], np.float32).reshape(H, W, 3)
        N = np.ascontiguousarray(feat["normal"], np.float32).reshape(H, W, 3)
        hit = np.ascontiguousarray(feat["hit_index"], np.int32).reshape(H, W) >= 0
        h = np.zeros((H, W, 8), np.float32)
        have = np.zeros((H, W), bool)
        if self.Hrec is None:                                                      # 1. first frame
            pass
        elif np.array_equal(cam.view(np.uint32), self.cam.view(np.uint32)):        # 2. static camera
            have = self.Hrec[..., 3] > 0
            h = np.where(have[..., None], self.Hrec, F32(0)).astype(np.float32)
        else:
            have, h = self._reproject(cam, P, N, hit, sigma_plane, min_normal_dot)
        hL = h[..., 7]                                                             # 5. cap
        capped = have & (hL > max_frames)
        k = np.where(capped, max_frames / np.where(capped, hL, F32(1)), F32(1)).astype(np.float32)
        h = np.where(capped[..., None], h * k[..., None], h).astype(np.float32)
        hs, hn, hs2, hL = h[..., 0:3], h[..., 3], h[..., 4:7], h[..., 7]
        cf = c.astype(np.float32)
        rec = np.empty((H, W, 8), np.float32)                                      # 6. merge and store
        rec[..., 0:3] = np.where(have[..., None], s + hs, s)
        rec[..., 3] = np.where(have, cf + hn, cf)
        rec[..., 4:7] = np.where(have[..., None], s2 + hs2, s2)
        rec[..., 7] = np.where(have, F32(1) + hL, F32(1))
        self.Hrec, self.P, self.N, self.hit, self.cam = rec, P.copy(), N.copy(), hit.copy(), cam
        pos = have & (hn > 0)                                                      # 7. outputs with an integer count
        n_i = np.where(pos, np.maximum(1, (np.where(pos, hn, F32(0)) + F32(0.5)).astype(np.int32)), 0).astype(np.int32)
        r = np.where(n_i > 0, n_i.astype(np.float32) / np.where(n_i > 0, hn, F32(1)), F32(1)).astype(np.float32)
        out_s = np.where(have[..., None], s + hs * r[..., None], s).astype(np.float32)
        out_s2 = np.where(have[..., None], s2 + hs2 * r[..., None], s2).astype(np.float32)
        return {"sum": out_s.reshape(-1, 3), "sum2": out_s2.reshape(-1, 3), "count": (c + n_i).astype(np.int32).reshape(-1),
                "history_frames": rec[..., 7].reshape(-1).copy()}

    def _reproject(self, cam, P, N, hit, sigma_plane, min_normal_dot):
        W, H = self.W, self.H
        inv = camera_inverse(self.cam)
        ys, xs = np.mgrid[0:H, 0:W]
        u = (xs.astype(np.float64) / W - 0.5).astype(np.float32)                   # 3. where was this pixel?
        v = (-ys.astype(np.float64) / H + 0.5).astype(np.float32)
        sky = (u[..., None] * cam[1] + v[..., None] * cam[2]) + cam[3]
        e = np.where(hit[..., None], P - self.cam[0], sky).astype(np.float32)
        a, b, g = (_dot(np.broadcast_to(inv[i], e.shape), e) for i in range(3))
        fw, fh = F32(W), F32(H)
        with np.errstate(all="ignore"):
            ok = g > 0
            gs = np.where(ok, g, F32(1))
            fx = (a / gs + F32(0.5)) * fw
            fy = (F32(0.5) - b / gs) * fh
            ok = ok & (fx >= -1) & (fx < fw) & (fy >= -1) & (fy < fh)
        fx, fy = np.where(ok, fx, F32(0)), np.where(ok, fy, F32(0))
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        Wt = np.zeros((H, W), np.float32)                                          # 4. which taps count?
        A = np.zeros((H, W, 8), np.float32)
        for j in (0, 1):
            for i in (0, 1):
                xq, yq = x0 + i, y0 + j
                inside = (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
                xc, yc = np.clip(xq, 0, W - 1), np.clip(yq, 0, H - 1)
                w = ((tx if i else F32(1) - tx) * (ty if j else F32(1) - ty)).astype(np.float32)
                rq = self.Hrec[yc, xc]
                use = ok & inside & (rq[..., 3] > 0) & (self.hit[yc, xc] == hit)
                dn = _dot(N, self.N[yc, xc])
                dist = np.abs(_dot(N, self.P[yc, xc] - P))
                use = use & (~hit | ((dn >= min_normal_dot) & (dist <= sigma_plane)))
                Wt = np.where(use, Wt + w, Wt)
                A = np.where(use[..., None], A + w[..., None] * rq, A).astype(np.float32)
        have = Wt > MIN_WEIGHT
        h = np.where(have[..., None], A / np.where(have, Wt, F32(1))[..., None], F32(0)).astype(np.float32)
        return have, h
