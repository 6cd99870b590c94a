"""Data shared by the float statistics tests (test_float_stats_host.py, test_gpu_float_stats.py):
the records of the radix select and its numpy counting step."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
DENORMAL = np.float32(1e-45)


def select_cases(n: int, seed: int = 5):
    """{label: float32 record of n elements} for the k-th smallest |x|: half exact zeros, -0.0,
    denormals, many duplicates at the selected value, one distinct value."""
    rng = np.random.default_rng(seed)
    normal = rng.standard_normal(n).astype(np.float32)
    relu = np.maximum(normal, 0).astype(np.float32)
    relu[::2] = 0
    signed_zero = normal.copy()
    signed_zero[::3] = -0.0
    signed_zero[1::3] = 0.0
    tiny = (rng.integers(-200, 200, n).astype(np.float32) * DENORMAL).astype(np.float32)
    tiny[::5] = normal[::5] * np.float32(1e-38)
    # the largest values are all equal: every k of the tests' falls on a duplicate at the top
    dup = np.minimum(np.abs(normal), np.float32(0.5)).astype(np.float32) * np.sign(normal).astype(np.float32)
    wide = (normal * np.float32(1e30)).astype(np.float32)
    wide[0], wide[-1] = FLT_MAX, -FLT_MAX
    return {"normal": normal, "relu": relu, "signed_zero": signed_zero, "denormal": tiny, "duplicates": dup,
            "constant": np.full(n, -3.25, np.float32), "wide": wide}


def numpy_digits(x: np.ndarray, level: int, prefix: int) -> np.ndarray:
    """What one record contributes to tk_fstats_plan_digits: 2048 counts (levels 1, 2: 1024 used)."""
    m = np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)
    if level == 0:
        digit = m >> np.uint32(20)
    elif level == 1:
        digit = (m[(m >> np.uint32(20)) == np.uint32(prefix)] >> np.uint32(10)) & np.uint32(1023)
    else:
        digit = m[(m >> np.uint32(10)) == np.uint32(prefix)] & np.uint32(1023)
    return np.bincount(digit.astype(np.int64), minlength=2048).astype(np.uint64)


def numpy_digit_counter(records):
    """radix_select's counting step over host records."""
    def count(level, prefixes):
        prefixes = [0] * len(records) if prefixes is None else prefixes
        return [numpy_digits(x, level, p)[:2048 if level == 0 else 1024] for x, p in zip(records, prefixes)]
    return count
