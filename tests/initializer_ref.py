"""The generator and the draw of mvSets as include/hs_twoview.h states them ("Generator", "Draw of mvSets"), in plain
Python: what hs_twoview_draw / hs_twoview_fit_flow_drawn are held to, bit for bit.  Parity with OpenCV's cv::RNG is
not pinned (OpenCV is not a dependency); the known answers in tests/test_initializer.py come from this definition."""
import numpy as np

M32 = 0xFFFFFFFF
MULT = 4164903690


class CvRng:
    def __init__(self, seed: int = 0):
        self.state = seed if seed else M32

    def next(self) -> int:
        self.state = ((self.state & M32) * MULT + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & M32

    def uniform(self, a: int, b: int) -> int:
        """[a, b): b is exclusive; a == b consumes no draw."""
        return a if a == b else int(self.next() % (b - a) + a)

    def skip(self, n: int):
        for _ in range(n):
            self.next()


def draw_sets_cv(status, n_sets: int, rng: CvRng) -> np.ndarray:
    """sets[n_sets][8]: per set 8 draws without replacement from the keys with status != 0 by swap-and-pop: the drawn
    slot takes the last available index, the list shrinks by one.  The generator runs on through all sets."""
    all_idx = [int(i) for i in np.flatnonzero(np.asarray(status) != 0)]
    m = len(all_idx)
    if m < 8:
        raise ValueError("fewer than 8 keys with status != 0")
    sets = np.zeros((n_sets, 8), np.int32)
    for it in range(n_sets):
        avail = list(all_idx)
        for j in range(8):
            size = m - j
            r = rng.uniform(0, size - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[size - 1]
            avail.pop()
    return sets
