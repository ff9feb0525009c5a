"""NumPy statements of the online multichannel Wiener filter of ``dcs_mwf_online_push_f32`` (include/dcs.h has the
recurrence): the filter of tests/mwf_ref.py with the sum over every frame of the file replaced by a running, optionally
forgetting, sum over the frames so far -- one Hermitian 2x2 state per (source, bin).

``mwf_online_em`` follows ``mwf_ref.mwf_em``: ``np.linalg.inv`` and einsums over generic 2x2 matrices, in float64 (the
oracle) or, with ``precision="c64"``, in complex64 / float32 throughout (the yardstick the GPU tests take their bound from).
It takes and returns the state, so that it can be driven in cuts.  ``mwf_online_closed`` is a second float64 restatement:
closed forms (adjugate over determinant, no normalisation) on scalar components, ``S - (S P) S`` instead of ``(I - W) S``.
``make_masked_case`` is the channel stream's situation: every estimate is a mask times the same mixture magnitudes.
"""
import numpy as np

from mwf_ref import make_case


def mwf_online_em(mag, phase, A, niter, forget=1.0, loading=1e-3, eps=1e-10, precision="f64", state=None):
    """mag, phase ``[2, T, F]`` (the mixture), A ``[2, J, T, F]`` (source magnitudes, already divided by ``pre_div``), state
    ``[J, F, 2, 2]`` complex (``None``: the first frame is absolute frame 0 and reads no state) -> the source images y
    ``[2, J, T, F]``, complex, and the state after the last frame (``niter = 0`` keeps none and hands ``state`` back)."""
    rdt, cdt = (np.float64, np.complex128) if precision == "f64" else (np.float32, np.complex64)
    ph = np.asarray(phase).astype(rdt)
    unit = (np.cos(ph) + np.asarray(1j, dtype=cdt) * np.sin(ph)).astype(cdt)                    # [2, T, F]
    x = (np.asarray(mag).astype(rdt) * unit).transpose(1, 2, 0)                                  # [T, F, 2]
    y0 = (np.asarray(A).astype(rdt) * unit[:, None]).transpose(2, 1, 3, 0)                       # [T, J, F, 2]
    T, J, F = y0.shape[:3]
    eye = np.eye(2, dtype=cdt)
    eps, half, forget, loading, one = rdt(eps), rdt(0.5), rdt(forget), rdt(loading), rdt(1)
    out = np.empty((T, J, F, 2), dtype=cdt)
    if int(niter) == 0:
        return y0.transpose(3, 1, 0, 2), state
    S = None if state is None else np.asarray(state).astype(cdt)
    for t in range(T):
        y = y0[t]
        C = y[..., :, None] * y[..., None, :].conj()                                             # [J, F, 2, 2]
        v = np.einsum("jfii->jf", C).real * half
        G = np.zeros((J, F, 2, 2), dtype=cdt) if S is None else forget * S
        for _ in range(int(niter)):
            N = G + C
            n = np.einsum("jfii->jf", N).real * half
            R = (N + (loading * n)[..., None, None] * eye) / ((one + loading) * n + eps)[..., None, None]
            Sv = v[..., None, None] * R                                                          # v_j R_j
            Cx = Sv.sum(axis=0) + eps * eye                                                      # [F, 2, 2]
            W = np.einsum("jfab,fbc->jfac", Sv, np.linalg.inv(Cx))
            y = np.einsum("jfab,fb->jfa", W, x[t])
            C = y[..., :, None] * y[..., None, :].conj() + np.einsum("jfab,jfbc->jfac", eye - W, Sv)
            v = np.einsum("jfii->jf", C).real * half
            assert C.dtype == cdt and v.dtype == rdt and y.dtype == cdt
        S = G + C
        out[t] = y
    return out.transpose(3, 1, 0, 2), S


def mwf_online_closed(mag, phase, A, niter, forget=1.0, loading=1e-3, eps=1e-10):
    """The same recurrence in float64 on scalar components ``[J, F]``: a, d real, b complex for every Hermitian matrix."""
    ph = np.asarray(phase).astype(np.float64)
    unit = np.exp(1j * ph)
    x = np.asarray(mag).astype(np.float64) * unit                                                # [2, T, F]
    y0 = np.asarray(A).astype(np.float64) * unit[:, None]                                        # [2, J, T, F]
    _, J, T, F = y0.shape
    out = np.array(y0)
    if int(niter) == 0:
        return out
    Sa = Sd = np.zeros((J, F))
    Sb = np.zeros((J, F), dtype=np.complex128)
    for t in range(T):
        y_0, y_1 = y0[0, :, t], y0[1, :, t]
        x0, x1 = x[0, t], x[1, t]
        Ca, Cd, Cb = np.abs(y_0) ** 2, np.abs(y_1) ** 2, y_0 * y_1.conj()
        v = (Ca + Cd) / 2
        Ga, Gd, Gb = forget * Sa, forget * Sd, forget * Sb
        for _ in range(int(niter)):
            Na, Nd, Nb = Ga + Ca, Gd + Cd, Gb + Cb
            n = (Na + Nd) / 2
            den = n + (loading * n + eps)
            sa, sd, sb = v * (Na + loading * n) / den, v * (Nd + loading * n) / den, v * Nb / den    # v_j R_j
            xa, xd, xb = sa.sum(axis=0) + eps, sd.sum(axis=0) + eps, sb.sum(axis=0)
            det = xa * xd - (xb * xb.conj()).real
            pa, pd, pb = xd / det, xa / det, -xb / det                                           # Cx^-1 = [[pa, pb], [pb*, pd]]
            # W = S P
            w00, w01 = sa * pa + sb * pb.conj(), sa * pb + sb * pd
            w10, w11 = sb.conj() * pa + sd * pb.conj(), sb.conj() * pb + sd * pd
            y_0, y_1 = w00 * x0 + w01 * x1, w10 * x0 + w11 * x1
            # C = y y^H + S - W S
            Ca = np.abs(y_0) ** 2 + (sa - (w00 * sa + w01 * sb.conj()).real)
            Cd = np.abs(y_1) ** 2 + (sd - (w10 * sb + w11 * sd).real)
            Cb = y_0 * y_1.conj() + (sb - (w00 * sb + w01 * sd))
            v = (Ca + Cd) / 2
        Sa, Sd, Sb = Ga + Ca, Gd + Cd, Gb + Cb
        out[0, :, t], out[1, :, t] = y_0, y_1
    return out


def make_masked_case(J, T, F, seed):
    """``make_case``'s mixture with estimates ``mask_j * mag[c]``: J masks that sum to one per (frame, bin), the same on both
    channels.  Returns float32 mag, phase ``[2, T, F]``, A ``[2, J, T, F]`` and the true images (complex128)."""
    mag, phase, _, img = make_case(J, T, F, seed=seed)
    rs = np.random.RandomState(seed + 1000)
    m = rs.rand(J, T, F) ** 2 + 1e-3
    m /= m.sum(axis=0)
    A = (m[None] * mag[:, None].astype(np.float64)).astype(np.float32)
    return mag, phase, A, img


def sdr(y, img):
    """10 log10 of the true images' energy over the error's, all sources and channels together."""
    return float(10 * np.log10((np.abs(img) ** 2).sum() / (np.abs(y - img) ** 2).sum()))


EPS = 1e-10
FORGETS = (1.0, 0.9)


def gpu_cases():
    """name -> dict(mag, phase [2,T,F], A [2,J,T,F] as handed to the call, ld, pre_div, eps, runs): the cases of
    tests/test_gpu_mwf_online.py.  ``runs`` lists (niter, forget, loading, oracle); ``oracle=False`` marks a run where the
    float64 oracle itself is not trustworthy (loading 0 on masked estimates: its two restatements differ by up to 3e-2; an
    eps whose square underflows) and only properties are tested."""
    cases = {}

    def add(name, J, T, F, ld, niters, seed=1, dual_mono=False, pre_div=1.0, eps=EPS, masked=False, loadings=(1e-3,), oracle=True):
        if masked:
            mag, phase, A, _ = make_masked_case(J, T, F, seed=seed)
        else:
            mag, phase, A, _ = make_case(J, T, F, seed=seed, dual_mono=dual_mono)
        runs = [(n, fg, ld_, oracle) for n in niters for fg in FORGETS for ld_ in loadings]
        cases[name] = dict(mag=mag, phase=phase, A=A, ld=ld, pre_div=pre_div, eps=eps, runs=runs)
        return cases[name]

    add("panned3", 3, 37, 70, 72, (0, 1, 2, 5), loadings=(1e-3, 1e-2))
    add("masked4", 4, 37, 65, 65, (1, 2, 5), masked=True)["runs"].append((2, 1.0, 0.0, False))
    add("dualmono3", 3, 37, 70, 72, (2,), dual_mono=True)
    add("one_source_masked", 1, 37, 70, 72, (2,), seed=2, masked=True)["runs"].append((2, 1.0, 0.0, False))
    for J, seed in ((5, 9), (6, 10), (7, 11), (8, 8)):       # across whatever register variant the kernel switches on
        add("sources%d" % J, J, 37, 70, 72, (2,), seed=seed)
    add("one_frame", 3, 1, 70, 72, (2,), seed=3)
    add("one_bin", 3, 37, 1, 3, (2,), seed=4)
    add("pre_div", 3, 37, 70, 72, (2,), seed=5, pre_div=0.3)
    add("long", 2, 700, 2, 2, (2,), seed=7)
    z = add("zeros", 3, 37, 70, 72, (2,), seed=6)
    for sl in (slice(0, 5), slice(20, 25)):                   # frames where mixture and estimates are all zero ...
        z["mag"][:, sl] = 0
        z["phase"][:, sl] = 0
        z["A"][:, :, sl] = 0
    z["A"][:, 1] = 0                                          # ... and a source that is zero everywhere
    # the same with an eps whose square underflows: properties only
    cases["zeros_tiny_eps"] = dict(z, eps=1e-200, runs=[(n, fg, ld_, False) for n, fg, ld_, _ in z["runs"]])
    return cases


def run_key(name, niter, forget, loading):
    return "%s@%d/%g/%g" % (name, niter, forget, loading)
