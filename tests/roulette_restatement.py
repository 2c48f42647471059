"""THE STEP of Russian roulette (pt_hip.h: Russian roulette) in numpy, from the header's text: float32 operations rounded once in the
order written.  tests/roulette_composition.py puts it into the frame; tests/test_roulette_host.py holds pt_roulette_step to it bit for
bit.  The keywords are the single errors of the discrimination test."""
import numpy as np

import glass_restatement as G
import grain_restatement as GR
import view_composition as V

F32 = np.float32
STREAM = 5
MIN_FLOOR, DEFAULT_FLOOR = F32(2.0 ** -10), F32(1.0 / 16.0)


def words(pixel, pass_, depth, seed):
    """w0 of philox(pixel, pass, depth, 5) under the integrator's key, depth as before the increment."""
    w = GR.philox(np.asarray(pixel, np.uint32), pass_, np.asarray(depth, np.uint32), STREAM, seed, V.PHILOX_KEY1)
    return np.asarray(w[0], np.uint32)


def step(throughput, w0, floor, *, undivided=False, unfloored_divide=False, inverted=False):
    """(T after the step [n, 3], survives [n], the word was used [n])."""
    t = np.array(throughput, F32).reshape(-1, 3)
    floor = F32(floor)
    with np.errstate(all="ignore"):
        m = np.maximum(np.maximum(np.abs(t[:, 0]), np.abs(t[:, 1])), np.abs(t[:, 2])).astype(F32)      # (np.maximum propagates a NaN)
        plays = m < F32(1)                                                                              # !(m < 1): survives unchanged
        p = np.where(m < floor, floor, m).astype(F32)
        u = G.unit_float(np.asarray(w0, np.uint32))
        wins = u < p
        if inverted:
            wins = ~wins
        by = m if unfloored_divide else p
        out = t.copy()
        q = plays & wins
        if not undivided:
            out[q] = (t[q] / by[q][:, None]).astype(F32)
        out[plays & ~wins] = F32(0)
    return out, ~plays | wins, plays
