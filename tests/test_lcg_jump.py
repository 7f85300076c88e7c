"""The decoder kernel's dropout streams (csrc/dec_w.hip: decw_step) are 24-bit linear congruential generators, x <- x[23:0] * A + C_i, whose
32-bit result is the word of two 16-bit uniforms a site consumes.  A reference-line tile that skips its m2m sub-block (a padded line: the step
discards what it would compute) moves each of its four streams past the draws it did not make with ONE step of the same shape,
x <- x[23:0] * A^n + C_i (A^n - 1) / (A - 1)  (decw_jump).  Restated here in integers: the jump agrees with n single steps in the 24 state
bits, and the next single step from either state yields the same 32-bit word -- so every later dropout decision of the launch is unchanged
(bits 31..24 of the stored word differ; the next step masks them)."""
import numpy as np
import pytest

A = 214013
C = (2531011, 1013904223 & 0xFFFFFF, 12345, 7046029)        # the four increments of a lane's streams (dec_w.hip: draw2)
M2M_STEPS = 6                                               # self_attention: 2 keep2 steps per stream; residual: 4 draw2 steps per stream
M32, M24 = 0xFFFFFFFF, 0xFFFFFF


def step(x, c):
    return ((x & M24) * A + c) & M32


def jump_constants(n, c):
    """decw_jump_mul / decw_jump_add: A^n and C (1 + A + ... + A^(n-1)), both mod 2^24, by the kernel's own recurrences."""
    a, g = 1, 0
    for _ in range(n):
        a = (a * A) & M24
        g = (g * A + c) & M24
    return a, g


def jump(x, n, c):
    a, g = jump_constants(n, c)
    return ((x & M24) * a + g) & M32


def test_jump_constants_are_the_closed_form():
    for c in C:
        for n in (1, 2, M2M_STEPS, 17):
            a, g = jump_constants(n, c)
            assert a == pow(A, n, 1 << 24)
            # (A^n - 1) / (A - 1) = 1 + A + ... + A^(n-1): the division is exact over the integers
            assert g == (c * ((A ** n - 1) // (A - 1))) % (1 << 24)
            assert a < (1 << 24) and g < (1 << 24)              # both factors of the multiply stay 24-bit operands


@pytest.mark.parametrize("n", [1, 2, 4, M2M_STEPS, 24])
def test_jump_equals_n_single_steps(n):
    rng = np.random.default_rng(20240 + n)
    states = rng.integers(0, 1 << 32, size=10_000, dtype=np.uint64)
    states[:4] = (0, M32, M24, 1 << 24)
    for i, c in enumerate(C):
        for x0 in states[i::4].tolist():                        # 2 500 states per stream: 10 000 in all
            x = x0
            for _ in range(n):
                x = step(x, c)
            y = jump(x0, n, c)
            assert (x & M24) == (y & M24), (hex(x0), i)
            assert step(x, c) == step(y, c), (hex(x0), i)       # the next word of two uniforms: all 32 bits


def test_vectorised_restatement_over_all_streams():
    """The same statement for 10 000 states on every stream at once (uint64 arithmetic, no overflow: both factors are below 2^24)."""
    rng = np.random.default_rng(7)
    x0 = rng.integers(0, 1 << 32, size=10_000, dtype=np.uint64)
    for c in C:
        x = x0.copy()
        for _ in range(M2M_STEPS):
            x = ((x & np.uint64(M24)) * np.uint64(A) + np.uint64(c)) & np.uint64(M32)
        a, g = jump_constants(M2M_STEPS, c)
        y = ((x0 & np.uint64(M24)) * np.uint64(a) + np.uint64(g)) & np.uint64(M32)
        assert np.array_equal(x & np.uint64(M24), y & np.uint64(M24))
        nx = ((x & np.uint64(M24)) * np.uint64(A) + np.uint64(c)) & np.uint64(M32)
        ny = ((y & np.uint64(M24)) * np.uint64(A) + np.uint64(c)) & np.uint64(M32)
        assert np.array_equal(nx, ny)
