"""What tests/test_stream_hold.py (GPU) and tests/test_stream_hold_host.py (CPU) share: THE hold schedule -- which clips of a B = 3
session take a hop at each tick (``step(frames, clips=...)``), explicit and deterministic -- and its restatement as launches.  A helper
module like primeref.py (not a conftest).

A tick whose list is empty advances nobody and launches nothing, so launch indices count the non-empty ticks.  (A waveform session's
first call launches nothing either; the properties test_stream_hold_host.py asserts are those of a spectral session.)"""
B = 3
# tick -> the clips that have a frame
TICKS = [
    [1, 2],     # 0   launch 0: clip 0 is held before it has ever run (the session's first launch / first waveform call)
    [1, 2],     # 1   launch 1: ... and again: two launches in a row, an even and an odd one
    [0, 1, 2],  # 2
    [0],        # 3   launch 3: clips 1 and 2 held (odd)
    [0],        # 4   launch 4: ... and again (even)
    [],         # 5   nobody: no launch
    [0, 1, 2],  # 6   launch 5
    [0, 2],     # 7   launch 6: clip 1 held between two active launches
    [0, 1, 2],  # 8
    [1, 2],     # 9   launch 8: clip 0 held
    [0, 1],     # 10  launch 9: clip 2 held in the very launch that would have restarted it (RESET_BEFORE)
    [0, 1, 2],  # 11  five ticks of everybody: the deep filter's reach (D = 2) and the waveform delay line (3 calls) run out
    [0, 1, 2],  # 12
    [0, 1, 2],  # 13
    [0, 1, 2],  # 14
    [0, 1, 2],  # 15
]
RESET_BEFORE = {10: [2]}  # tick -> reset(clips=...) issued right before it


def launches():
    """[(tick, launch index, active clips, held clips)] of the ticks that launch."""
    out = []
    for t, active in enumerate(TICKS):
        if active:
            out.append((t, len(out), list(active), [b for b in range(B) if b not in active]))
    return out


def feed():
    """[(tick, {clip: j})]: clip b's j-th active tick (j counts from 0 over the whole schedule; the clip is fed its frames
    [j * hop, (j + 1) * hop) -- or its j-th block of 128 samples)."""
    seen = [0] * B
    out = []
    for t, active in enumerate(TICKS):
        out.append((t, {b: seen[b] for b in active}))
        for b in active:
            seen[b] += 1
    return out


def active_ticks():
    """Per clip, the number of ticks it takes."""
    return [sum(b in a for a in TICKS) for b in range(B)]


def resets():
    """{clip: j}: the clip is reset when it has taken j ticks (a control that steps every clip every time resets it before call j)."""
    out = {}
    for t, fed in feed():
        for b in RESET_BEFORE.get(t, []):
            out[b] = sum(b in a for a in TICKS[:t])
    return out
