"""An extended-precision Kabsch update: the reference of the ICP update tests (icp_update_cases.py, test_icp_update_cpu.py,
test_gpu_icp_update.py).  The input is the fp64 pair set (p', q) - p' = icp_np.transform(T0, P) on the inliers, q their correspondences -
taken as exact numbers; everything after it runs in mpmath at 60 digits: the means, the centred H = sum (p' - mu_p)(q - mu_q)^T, its SVD
(mpmath.svd_r), dR = V diag(1, 1, sign det(V U^T)) U^T, dt = mu_q - dR mu_p and T1 = [dR R0 | dR t0 + dt], rounded to fp64 at the end.
No device arithmetic and no NumPy arithmetic is involved, so the result does not depend on the order of any sum."""
import mpmath
import numpy as np

DIGITS = 60


def _mat(a):
    a = np.asarray(a, np.float64)
    return mpmath.matrix([[mpmath.mpf(float(x)) for x in row] for row in a])


def _det3(m):
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def kabsch_update(p, q, T0):
    """p, q [n, 3] fp64 (n >= 1), T0 [3, 4] -> dict(T float64 [3, 4], s (s1, s2, s3) floats, d +1 | -1, mu_p, mu_q float64 [3])."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1, 3)
    n = len(p)
    with mpmath.workdps(DIGITS):
        P, Q = _mat(p), _mat(q)
        one = mpmath.matrix([[mpmath.mpf(1)] * n])
        mu_p, mu_q = (one * P) / n, (one * Q) / n                     # [1, 3]
        Pc = P - mpmath.matrix([[mu_p[0, k] for k in range(3)] for _ in range(n)])
        Qc = Q - mpmath.matrix([[mu_q[0, k] for k in range(3)] for _ in range(n)])
        H = Pc.T * Qc
        U, S, Vt = mpmath.svd_r(H)                                    # singular values descending
        V = Vt.T
        d = 1 if _det3(V * U.T) > 0 else -1
        dR = V * mpmath.diag([1, 1, d]) * U.T
        dt = mu_q.T - dR * mu_p.T
        T0m = _mat(np.asarray(T0, np.float64).reshape(3, 4))
        R1 = dR * T0m[:, 0:3]
        t1 = dR * T0m[:, 3] + dt
        T = np.array([[float(R1[a, b]) for b in range(3)] + [float(t1[a])] for a in range(3)])
        return dict(T=T, s=tuple(float(S[k]) for k in range(3)), d=d, ratio=float(S[1] / S[0]) if S[0] > 0 else 0.0,
                    mu_p=np.array([float(mu_p[0, k]) for k in range(3)]), mu_q=np.array([float(mu_q[0, k]) for k in range(3)]))
