"""NumPy float64 reference of the dense Adam step: tf.clip_by_norm per variable (train.py:134-135), then
Keras 2.12 ``tf.keras.optimizers.Adam.update_step`` per element.  ``step`` is the 1-based index of the step being
applied (Keras' ``iterations + 1``).  Note the epsilon OUTSIDE the square root (Keras RMSprop has it inside)."""

import numpy as np


def clip_by_norm(g, clip):
    """g * clip / max(||g||_2, clip); clip <= 0: no clipping."""
    g = np.asarray(g, np.float64)
    if clip <= 0:
        return g.copy()
    return g * clip / max(float(np.sqrt(np.sum(g * g))), clip)


def adam_update(w, g, m, v, lr, beta1, beta2, eps, step):
    """One Adam step on an (already clipped) gradient -> (w, m, v), float64."""
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    alpha = lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    m = m + (g - m) * (1.0 - beta1)
    v = v + (g * g - v) * (1.0 - beta2)
    w = w - (m * alpha) / (np.sqrt(v) + eps)
    return w, m, v


def seg_index(seg):
    """Flat indices of a segment {offset, rows, cols, row_stride}, row-major."""
    o, r, c, s = (int(x) for x in seg)
    return (o + np.arange(r)[:, None] * s + np.arange(c)[None]).reshape(-1)


def clip_adam(w, g, m, v, segs, lr, beta1, beta2, eps, step, clip):
    """ot_clip_adam on flat float64 buffers: every segment clipped by its own norm and updated; elements outside
    every segment come back as they went in.  Returns new (w, m, v)."""
    w, g, m, v = (np.array(a, np.float64) for a in (w, g, m, v))
    for seg in np.asarray(segs).reshape(-1, 4):
        idx = seg_index(seg)
        w[idx], m[idx], v[idx] = adam_update(w[idx], clip_by_norm(g[idx], clip), m[idx], v[idx], lr, beta1, beta2,
                                             eps, step)
    return w, m, v
