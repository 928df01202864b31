"""Planning of ragged batches: which utterances of different lengths travel together in one library call.

Pure host logic (no GPU, no library): a ragged call of a handle holds at most ``max_batch`` utterances and at most
``row_capacity`` frames in all (the rows of the workspace the handle owns, ``max_batch * T``); an utterance needs at least
``MIN_FRAMES`` frames (block 3 of ECAPA-TDNN reflect-pads 4).  An utterance that cannot ride in ANY call (longer than the whole
capacity, or too short) is handed back to the caller, which keeps the per-length handle for it.  RawNet3 counts the frames after its
sinc filterbank (at least 30); a fusion model plans both of its branches at once (FusionPacker).
"""
from __future__ import annotations

MIN_FRAMES = 5


class RaggedPacker:
    """Fills one call at a time.  ``add(frames)`` says whether the utterance still fits the call being filled; ``fits_alone``
    whether it fits an empty one."""

    def __init__(self, max_batch, row_capacity, min_frames=MIN_FRAMES):
        if max_batch < 1 or row_capacity < 1:
            raise ValueError("max_batch and row_capacity must be positive")
        self.max_batch, self.row_capacity, self.min_frames = int(max_batch), int(row_capacity), int(min_frames)
        self.reset()

    def reset(self):
        self.count = 0
        self.rows = 0

    def fits_alone(self, frames):
        return self.min_frames <= frames <= self.row_capacity

    def add(self, frames):
        if not self.fits_alone(frames) or self.count + 1 > self.max_batch or self.rows + frames > self.row_capacity:
            return False
        self.count += 1
        self.rows += int(frames)
        return True


def plan_ragged(frames, max_batch, row_capacity, min_frames=MIN_FRAMES):
    """frame counts, in file order -> (calls, alone).  ``calls``: lists of indices, each one library call that fits, the
    indices ascending within and across calls; ``alone``: the indices that fit no call.  Every index appears exactly once.
    Greedy and in order: a call is closed when the next utterance does not fit it."""
    packer = RaggedPacker(max_batch, row_capacity, min_frames)
    calls, alone, cur = [], [], []
    for i, t in enumerate(frames):
        t = int(t)
        if not packer.fits_alone(t):
            alone.append(i)
            continue
        if not packer.add(t):
            calls.append(cur)
            cur = []
            packer.reset()
            packer.add(t)
        cur.append(i)
    if cur:
        calls.append(cur)
    return calls, alone


class FusionPacker:
    """One plan for the two branches of a fusion model, which read the same waveforms: the unit is the pair (frames of the first
    branch, frames of the second), and a call is closed when EITHER branch's utterance count or row capacity would overflow."""

    def __init__(self, first, second):
        self.packers = (first, second)

    def reset(self):
        for p in self.packers:
            p.reset()

    def fits_alone(self, frames):
        return all(p.fits_alone(f) for p, f in zip(self.packers, frames))

    def add(self, frames):
        a, b = self.packers
        if not self.fits_alone(frames) or a.count + 1 > a.max_batch or a.rows + frames[0] > a.row_capacity \
                or b.count + 1 > b.max_batch or b.rows + frames[1] > b.row_capacity:
            return False
        return a.add(frames[0]) and b.add(frames[1])


def plan_packed(units, packer):
    """plan_ragged with a packer of any unit (RaggedPacker: frame counts; FusionPacker: pairs): -> (calls, alone)"""
    packer.reset()
    calls, alone, cur = [], [], []
    for i, t in enumerate(units):
        if not packer.fits_alone(t):
            alone.append(i)
            continue
        if not packer.add(t):
            calls.append(cur)
            cur = []
            packer.reset()
            packer.add(t)
        cur.append(i)
    if cur:
        calls.append(cur)
    packer.reset()
    return calls, alone
