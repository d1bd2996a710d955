"""The learning-rate schedule's definition in fp64 Python floats: the reference of the CPU and the GPU tests.

``s`` optimizer steps were already taken under the schedule (0 for the first); ``W`` warm-up steps, ``T`` total
steps, ``r`` the ratio the decay ends at.  The lr a step uses is ``base * factor(s)``.
"""
import math

KINDS = ("constant", "linear", "cosine", "poly")


def factor(s, kind, W, T, r=0.0, power=1.0):
    if s < W:
        return (s + 1) / W
    t = min(1.0, (s - W) / max(1, T - W))
    if kind == "constant":
        return 1.0
    if kind == "linear":
        return 1.0 - (1.0 - r) * t
    if kind == "cosine":
        return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * t))
    if kind == "poly":
        return r + (1.0 - r) * (1.0 - t) ** power
    raise ValueError(kind)


def lr(base, s, kind, W, T, r=0.0, power=1.0):
    return base * factor(s, kind, W, T, r, power)
