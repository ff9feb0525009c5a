"""NumPy statement of the multichannel Wiener filter of ``dcs_mwf_f32`` (include/dcs.h): the EM for full-rank, time-invariant
spatial covariances, two channels.  The reference's own ``mwf`` (util.py:633-719) never ran, so this is the oracle.

``mwf_em`` is written with ``np.linalg.inv`` and einsums over generic 2x2 matrices, independent of any closed form a
kernel uses.  It runs in float64 (the oracle) or, with ``precision="c64"``, in complex64 / float32 throughout -- the
yardstick the GPU tests take their bound from.  ``make_case`` is the seeded test signal.
"""
import numpy as np


def mwf_em(mag, phase, A, niter, eps=1e-10, precision="f64"):
    """mag, phase ``[2, T, F]`` (the mixture), A ``[2, J, T, F]`` (source magnitudes, already divided by ``pre_div``)
    -> the source images y ``[2, J, T, F]``, complex."""
    rdt, cdt = (np.float64, np.complex128) if precision == "f64" else (np.float32, np.complex64)
    ph = np.asarray(phase).astype(rdt)
    unit = (np.cos(ph) + np.asarray(1j, dtype=cdt) * np.sin(ph)).astype(cdt)                    # [2, T, F]
    x = (np.asarray(mag).astype(rdt) * unit).transpose(1, 2, 0)                                  # [T, F, 2]
    y = (np.asarray(A).astype(rdt) * unit[:, None]).transpose(1, 2, 3, 0)                        # [J, T, F, 2]
    eye = np.eye(2, dtype=cdt)
    eps = rdt(eps)
    half = rdt(0.5)
    C = y[..., :, None] * y[..., None, :].conj()                                                 # [J, T, F, 2, 2]
    v = np.einsum("jtfii->jtf", C).real * half
    for _ in range(int(niter)):
        R = C.sum(axis=1) / (v.sum(axis=1) + eps)[..., None, None]                               # [J, F, 2, 2]
        S = v[..., None, None] * R[:, None]                                                      # [J, T, F, 2, 2]
        Cx = S.sum(axis=0) + eps * eye                                                           # [T, F, 2, 2]
        W = np.einsum("jtfab,tfbc->jtfac", S, np.linalg.inv(Cx))
        y = np.einsum("jtfab,tfb->jtfa", W, x)
        C = y[..., :, None] * y[..., None, :].conj() + np.einsum("jtfab,jtfbc->jtfac", eye - W, S)
        v = np.einsum("jtfii->jtf", C).real * half
        assert C.dtype == cdt and v.dtype == rdt and y.dtype == cdt
    return y.transpose(3, 0, 1, 2)


def make_case(J, T, F, seed, dual_mono=False):
    """J sparse complex sources times per-bin gains, panned at ``linspace(0.15, 1.4, J)`` radians (all at pi / 4 for
    ``dual_mono``: both channels equal, Cx of rank 1 up to eps).  Estimates ``|image| * exp(0.5 N) + 0.1 |X| U``.
    Returns float32 mag, phase ``[2, T, F]``, A ``[2, J, T, F]`` and the true images ``[2, J, T, F]`` (complex128)."""
    rs = np.random.RandomState(seed)
    s = (rs.randn(J, T, F) + 1j * rs.randn(J, T, F)) * (rs.rand(J, T, F) < 0.3) * (0.2 + 2.0 * rs.rand(J, 1, F))
    theta = np.full(J, np.pi / 4) if dual_mono else np.linspace(0.15, 1.4, J)
    pan = np.stack([np.cos(theta), np.sin(theta)])                                               # [2, J]
    img = pan[:, :, None, None] * s[None]
    X = img.sum(axis=1)
    A = np.abs(img) * np.exp(0.5 * rs.randn(2, J, T, F)) + 0.1 * np.abs(X)[:, None] * rs.rand(2, J, T, F)
    return np.abs(X).astype(np.float32), np.angle(X).astype(np.float32), A.astype(np.float32), img


def mixture(mag, phase):
    return mag.astype(np.float64) * np.exp(1j * phase.astype(np.float64))


def polar(out_mag, out_phase):
    return out_mag.astype(np.float64) * np.exp(1j * out_phase.astype(np.float64))
