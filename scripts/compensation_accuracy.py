"""How accurately float32 computes the antialiasing compensation sqrt(det(cov2d) / det(cov2d + e I)), in the
two forms k_project_fwd could use, against fp64:

  det   the pre-blur determinant, as the kernel computes it: fma(-c01, c01, c00 c11) / ((c00 + e)(c11 + e) - c01^2)
  conic 1 - e (qa + qc) + e^2 (qa qc - qb^2) from the stored float32 conic (qa, qb, qc) = inv(cov2d + e I)

cov2d is a rotated diag(l1, l2) per sample.  Two references: fp64 from the float32-rounded cov2d (the error of the formula alone) and
fp64 from the exact cov2d (what a float32 cov2d can reach at all).  CPU only, numpy; an fma is emulated in float64 (a product of two
float32 values is exact there) with one rounding to float32.

  python scripts/compensation_accuracy.py [--n 200000] [--eps 0.3]"""
import argparse

import numpy as np

f32 = np.float32


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def forms(c00, c01, c11, e):
    e = f32(e)
    a, b, c = c00 + e, c01, c11 + e
    det = fma32(a, c, -(b * b))  # the classic det as the kernel's contraction computes it
    ok = det > 0
    det0 = fma32(-c01, c01, c00 * c11)
    m_det = np.sqrt(np.maximum(f32(0), det0 / det))
    idet = f32(1) / det
    qa, qb, qc = c * idet, -b * idet, a * idet
    m_con = np.sqrt(np.maximum(f32(0), f32(1) - e * (qa + qc) + e * e * (qa * qc - qb * qb)))
    return ok, m_det, m_con


def truth(c00, c01, c11, e):
    d0 = c00 * c11 - c01 * c01
    d1 = (c00 + e) * (c11 + e) - c01 * c01
    return np.sqrt(np.maximum(0.0, d0 / d1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--eps", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    print(f"{'l1':>8} {'l2':>8} {'comp':>17} | max abs error vs fp64 of the rounded cov2d: det  conic | vs the exact cov2d: det  conic")
    for l1, l2 in [(1, 1), (100, 1), (100, 1e-2), (1e3, 1e-3), (1e4, 1e-4), (10, 1e-6), (1e4, 1e-6)]:
        th = rng.uniform(0, np.pi, a.n)
        cs, sn = np.cos(th), np.sin(th)
        c00, c11, c01 = l1 * cs * cs + l2 * sn * sn, l1 * sn * sn + l2 * cs * cs, (l1 - l2) * cs * sn
        C00, C01, C11 = c00.astype(f32), c01.astype(f32), c11.astype(f32)
        ok, m_det, m_con = forms(C00, C01, C11, a.eps)
        t_r = truth(C00.astype(np.float64), C01.astype(np.float64), C11.astype(np.float64), a.eps)[ok]
        t_x = truth(c00, c01, c11, a.eps)[ok]
        err = lambda m, t: float(np.abs(m[ok] - t).max())
        print(f"{l1:8.0e} {l2:8.0e} {t_x.min():8.2e}-{t_x.max():8.2e} | {err(m_det, t_r):8.2e} {err(m_con, t_r):8.2e} | "
              f"{err(m_det, t_x):8.2e} {err(m_con, t_x):8.2e}")


if __name__ == "__main__":
    main()
