"""The frame of a scene under an ENVIRONMENT (pt_hip.h: pt_environment_*), composed on the host from the CPU oracle's parts:
tests/projection_composition.compose with one change -- before Scene.segments, a ray whose closest hit is a miss contributes
col * lookup(direction) (tests/environment_restatement.py), counts one and ends.  The primary ray is any view's: the pinhole and the
projections (projection_composition), the thin lens (view_composition) and the moving camera (motion_composition)."""
import numpy as np

import environment_restatement as E
import motion_composition as M
import oracle_lib as O
import projection_composition as P
import view_composition as V

F32 = np.float32


def compose(scene, env_map, width, height, pixels, spp, mrr, *, camera=None, projection=(P.PERSPECTIVE, 0.0, 0.0), lens=None, motion_end=None,
            seed=42, eps=1e-4, error=-1.0, pass_begin=0):
    """sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)) after passes pass_begin ..
    pass_begin + spp - 1 under the (N, N, 3) octahedral map `env_map`.  `scene` None = the empty scene: every ray misses."""
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    n = len(px)
    gpix = (px[:, 1] * width + px[:, 0]).astype(np.uint32)
    s, s2, cnt = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, np.int32)
    for p in range(pass_begin, pass_begin + spp):
        skip = O.adaptive_skip(np.full(n, p, np.int32), s, s2, cnt, error)
        act = np.nonzero(~skip)[0]
        if len(act) == 0:
            continue
        words = V.philox(gpix[act], p, 0xFFFFFFFF, seed)
        if motion_end is not None:
            o, d = M.primary_rays(px[act, 0], px[act, 1], width, height, words, M.shutter_time(gpix[act], p, seed), camera, motion_end, lens=lens)
        elif lens is not None:
            o, d = V.primary_rays(px[act, 0], px[act, 1], width, height, words, camera, lens)
        else:
            o, d = P.primary_rays(px[act, 0], px[act, 1], width, height, words, camera, projection)
        col = np.ones((len(act), 3), F32)
        depth = np.zeros(len(act), np.int32)
        live = np.arange(len(act))
        while len(live):
            if scene is None:
                miss = np.ones(len(live), bool)
            else:
                miss = scene.closest_hits(o[live], d[live], eps=eps)[0] < 0
            if miss.any():                       # the restated miss: throughput x L(direction), one contribution, the path ends
                m = live[miss]
                with np.errstate(all="ignore"):
                    c = (col[m] * E.lookup(env_map, d[m])).astype(F32)
                    s[act[m]] += c
                    s2[act[m]] += c * c
                cnt[act[m]] += 1
                live = live[~miss]
                if not len(live):
                    break
            w = V.philox(gpix[act[live]], p, depth[live], seed)[:, :3]
            o2, d2, c2, dep2, contrib, did = scene.segments(o[live], d[live], col[live], depth[live], w, eps=eps, mrr=mrr, trig=O.TRIG_PORTABLE)
            o[live], d[live], col[live], depth[live] = o2, d2, c2, dep2
            k = act[live[did]]
            with np.errstate(all="ignore"):
                s[k] += contrib[did]
                s2[k] += contrib[did] * contrib[did]
            cnt[k] += 1
            live = live[(dep2 < mrr) & np.any(c2 != 0, axis=1)]
    return s, s2, cnt
