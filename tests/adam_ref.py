"""float64 NumPy restatement of lasagne.updates.adam (test infrastructure), the update csrc/train_core.hip's adam_kernel
applies:

    t   = t_prev + 1
    a_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
    m'  = beta1 * m + (1 - beta1) * g
    v'  = beta2 * v + (1 - beta2) * g * g
    p'  = p - a_t * m' / (sqrt(v') + epsilon)

epsilon is added outside the bias correction, which is not where torch.optim.Adam adds it (there the denominator is
sqrt(v' / (1 - beta2^t)) + epsilon); the two coincide as epsilon -> 0, which tests/test_train_schedules_cpu.py uses to pin
the recursion and the bias correction."""
import numpy as np

LR, BETA1, BETA2, EPSILON = 1e-3, 0.9, 0.999, 1e-8


def a_t(t, lr=LR, beta1=BETA1, beta2=BETA2):
    """The step size of step ``t`` (1 for the first)."""
    return lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def adam(params, grads, m, v, t_prev, lr=LR, beta1=BETA1, beta2=BETA2, epsilon=EPSILON):
    """One step on lists of arrays (float64): new params, m, v, and the steps taken (``t_prev`` + 1 is this step's t)."""
    t = t_prev + 1
    a = a_t(t, lr, beta1, beta2)
    P, M, V, S = [], [], [], []
    for p, g, mi, vi in zip(params, grads, m, v):
        g = np.asarray(g, np.float64)
        mi = beta1 * np.asarray(mi, np.float64) + (1 - beta1) * g
        vi = beta2 * np.asarray(vi, np.float64) + (1 - beta2) * g * g
        step = a * mi / (np.sqrt(vi) + epsilon)
        P.append(np.asarray(p, np.float64) - step)
        M.append(mi)
        V.append(vi)
        S.append(step)
    return P, M, V, S
