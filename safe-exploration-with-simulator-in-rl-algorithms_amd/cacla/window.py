"""Smoothing of learning curves: the mirror of the reference's cacla/window.py."""
import numpy as np


def window_convolution(a, H):
    """The averages of the last H values of a: [len(a) - H] (empty when len(a) <= H).  A running sum in the
    reference's order -- the value that leaves the window is subtracted, then the new one added -- so the results are
    the reference's bit for bit; a vectorised cumulative sum would round differently."""
    v = []
    sum_H = 0
    for i in range(len(a)):
        if i >= H:
            sum_H -= a[i - H]
            sum_H += a[i]
            v.append(sum_H)
        else:
            sum_H += a[i]
    return np.array(v) / H
