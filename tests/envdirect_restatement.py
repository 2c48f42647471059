"""Environment sampling restated in numpy from the text of include/pt_hip.h ("environment sampling": THE TABLE, SHARE, THE SAMPLE AND THE
TERM), operation by operation: the table and the share in float64 with the lookup of tests/environment_restatement.py, the sample and
the term float32 operations rounded once in the order the header writes them, nothing fused.  The keyword switches of `sample` and
`term` are the single errors tests/test_envdirect_host.py plants to show that the agreement in expectation tells them from the stated
arithmetic."""
import numpy as np

import direct_restatement as D
import environment_restatement as E
import glass_restatement as G
import grain_restatement as GR
import view_composition as V

F32 = np.float32
f32 = G.f32
PI = F32(3.141593)
RECORD = np.dtype([("accept", np.float32), ("alias", np.int32), ("pdf_self", np.float32), ("pdf_alias", np.float32)])


def lum(rgb):
    return (0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1]) + 0.0722 * rgb[..., 2]


def cell_weights(env_map):
    """(W [S * S] float64 before the floor, S) of an (N, N, 3) map."""
    n = env_map.shape[0]
    s = min(n, 256)
    k = max(2, -(-2 * n // s))
    w = np.zeros((s, s), np.float64)
    ci = np.arange(s, dtype=np.float64)
    rows = max(1, 4096 // (s * k * k))                                   # (rows of cells at a time: the N = 512 map has 4 M sub-points)
    for j0 in range(0, s, rows):
        cj = np.arange(j0, min(s, j0 + rows), dtype=np.float64)
        acc = np.zeros((len(cj), s), np.float64)
        for sj in range(k):
            for si in range(k):
                qx = np.broadcast_to(2.0 * ((ci + (si + 0.5) / k) / s) - 1.0, (len(cj), s))
                qz = np.broadcast_to((2.0 * ((cj + (sj + 0.5) / k) / s) - 1.0)[:, None], (len(cj), s))
                py = 1.0 - np.abs(qx) - np.abs(qz)
                up = py >= 0
                px = np.where(up, qx, np.copysign(1.0 - np.abs(qz), qx))
                pz = np.where(up, qz, np.copysign(1.0 - np.abs(qx), qz))
                ln = np.sqrt(px * px + py * py + pz * pz)
                d = np.stack([px / ln, py / ln, pz / ln], -1).astype(F32).reshape(-1, 3)
                L = E.lookup(env_map, d).astype(np.float64).reshape(len(cj), s, 3)
                L = np.where(L > 0, L, 0.0)
                acc += lum(L) / ((ln * ln) * ln)
        w[j0:j0 + len(cj)] = (4.0 / float(s * s)) * (acc / (k * k))
    return w.reshape(-1), s


def table(env_map):
    """(records [S * S] of RECORD, P [S * S] float64, Phi_env, S), or None where the map is refused."""
    w, s = cell_weights(np.ascontiguousarray(env_map, F32))
    cells = s * s
    phi = 0.0
    for x in w:
        phi += float(x)
    if not (phi > 0.0) or not np.isfinite(phi):
        return None
    floor_w = phi / float(cells) / 16.0
    w = np.where(w < floor_w, floor_w, w)
    total = 0.0
    for x in w:
        total += float(x)
    prob = w / total
    p = (prob * float(cells)).tolist()
    rec = np.zeros(cells, RECORD)
    rec["accept"] = 1.0
    rec["alias"] = np.arange(cells)
    rec["pdf_self"] = rec["pdf_alias"] = (prob * (float(cells) / 4.0)).astype(F32)
    small = [c for c in range(cells) if p[c] < 1.0]
    large = [c for c in range(cells) if not p[c] < 1.0]
    while small and large:
        sm, lg = small.pop(), large.pop()
        rec["accept"][sm] = F32(p[sm])
        rec["alias"][sm] = lg
        rec["pdf_alias"][sm] = rec["pdf_self"][lg]
        p[lg] = (p[lg] + p[sm]) - 1.0
        (small if p[lg] < 1.0 else large).append(lg)
    return rec, prob, phi, s


def default_share(phi_env, lights):
    """SHARE of a scene with the light table `lights` (tests/direct_restatement.light_table)."""
    if len(lights["area"]) == 0:
        return F32(1)
    total = 0.0
    for a, le in zip(lights["area"], lights["le"].astype(np.float64)):
        total += float(a) * float(lum(le))
    phi_em = 3.14159265358979323846 * total
    return F32(min(max(F32(phi_env / (phi_env + phi_em)), F32(0.125)), F32(0.875)))


def sample_words(pixel, pass_, depth, seed):
    """(e0, e1, e2, e3) = philox(pixel, pass, depth, 4) under the integrator's key."""
    w = GR.philox(np.asarray(pixel, np.uint32), pass_, np.asarray(depth, np.uint32), 4, seed, V.PHILOX_KEY1)
    return np.stack(w, 1).astype(np.uint32)


def sample(rec, s, e0, e1, e2, e3, *, drop_jacobian=False, self_pdf=False, skip_fold=False):
    """(cell, w [n, 3], pdf_w) of THE SAMPLE."""
    e0 = np.asarray(e0, np.uint32).astype(np.uint64)
    drawn = ((e0 * np.uint64(s * s)) >> np.uint64(32)).astype(np.int64)
    r = rec[drawn]
    keep = G.unit_float(e1) < r["accept"]
    c = np.where(keep, drawn, r["alias"]).astype(np.int64)
    pdf_q = np.where(keep | self_pdf, r["pdf_self"], r["pdf_alias"]).astype(F32)
    cj = c // s
    ci = c - cj * s
    cw = F32(2.0) / F32(s)
    with np.errstate(all="ignore"):
        qx = ((ci.astype(F32) + G.unit_float(e2)).astype(F32) * cw).astype(F32) - F32(1)
        qz = ((cj.astype(F32) + G.unit_float(e3)).astype(F32) * cw).astype(F32) - F32(1)
        ax, az = np.abs(qx), np.abs(qz)
        py = ((F32(1) - ax).astype(F32) - az).astype(F32)
        up = (py >= 0) | skip_fold
        px = np.where(up, qx, np.copysign(F32(1) - az, qx)).astype(F32)
        pz = np.where(up, qz, np.copysign(F32(1) - ax, qz)).astype(F32)
        p = np.stack([px, py, pz], 1).astype(F32)
        ln = np.sqrt(((px * px + py * py).astype(F32) + pz * pz).astype(F32)).astype(F32)
        w = G.normalize(p)
        pdf_w = pdf_q if drop_jacobian else (pdf_q * ((ln * ln).astype(F32) * ln).astype(F32)).astype(F32)
    return c.astype(np.int32), w, pdf_w


def term(env_map, w, pdf_w, share, N, n, T, kd, *, cs_twice=False, no_pi=False, keep_share=False):
    """(term [k, 3], has [k]) of THE TERM without the visibility."""
    N, n, T, kd = f32(N).reshape(-1, 3), f32(n).reshape(-1, 3), f32(T).reshape(-1, 3), f32(kd).reshape(-1, 3)
    share = F32(share)
    with np.errstate(all="ignore"):
        cn, cs = D.dot(N, w), D.dot(n, w)
        has = (cn > 0) & (cs > 0) & (pdf_w > 0) & (pdf_w < np.inf)
        L = E.lookup(env_map, w)
        num = (cs * cs).astype(F32) if cs_twice else (cs * np.abs(w[:, 2])).astype(F32)
        den = pdf_w if no_pi else (PI * pdf_w).astype(F32)
        den = den if keep_share else (den * share).astype(F32)
        g = (num / den).astype(F32)
        t = (((T * kd).astype(F32) * L).astype(F32) * g[:, None]).astype(F32)
    return np.where(has[:, None], t, F32(0)).astype(F32), has
