"""A numpy float32 restatement of the weight-averaging rule (tf.train.ExponentialMovingAverage without zero-debias): every operation
takes float32 operands and rounds its result to float32 once - what TensorFlow's assign_moving_average does on float32 variables and
what skf_ema.hip must reproduce bit for bit."""
import numpy as np

F = np.float32


def decay_at(decay, num_updates, iterations):
    """d = decay, or with num_updates min(decay, (1 + n) / (10 + n)) for n = float32(iterations) - tf casts num_updates to float32
    first, so beyond 2^24 n is the nearest float32 (2^24 + 1 -> 2^24)."""
    d = F(decay)
    if not num_updates:
        return d
    n = F(np.int64(iterations))
    return np.minimum(d, (F(1.0) + n) / (F(10.0) + n)).astype(F)[()]


def one_minus(d):
    return F(1.0) - F(d)


def update(shadow, w, omd):
    """shadow - (shadow - w) * omd on float32 arrays: subtract, multiply, subtract, each rounded once.  -> a new array"""
    shadow, w, omd = np.asarray(shadow, F), np.asarray(w, F), F(omd)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = shadow - w
        delta = diff * omd
        return shadow - delta
