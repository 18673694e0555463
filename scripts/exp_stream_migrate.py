"""Moving clips between streaming sessions: export_state, import_state and the pair against one step of the same session and against
the only alternative there was -- prime over the clip's whole recorded past, here 10 s (profiles/stream_migrate.md).  baseline_m,
one-launch tier, B = 16, one and eight clips moved to a second session; p50 / p99 of alternating iterations, host clock from a
synchronised stream to a synchronised stream.  Run on the MI355X box: python scripts/exp_stream_migrate.py [iterations] [out.md]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import refweights as rw
from test_hip_parity import build_module

DEV = torch.device("cuda:0")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else None
kw, B, N = rw.LIVE_M, 16, 1250  # 1250 frames = 10 s
model = build_module("live", kw, rw.live_state_dict(kw, 5))
rng = np.random.default_rng(7)
full = torch.from_numpy(((rng.standard_normal((B, 257, N)) + 1j * rng.standard_normal((B, 257, N))) * 0.5).astype(np.complex64)).to(DEV)
src, dst = model.streaming(batch=B), model.streaming(batch=B)
assert src._hop is not None
frames = [full[..., t:t + 1].contiguous() for t in range(40)]
for x in frames[:32]:
    src.step(x, copy=False), dst.step(x, copy=False)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def pct(v):
    v = np.asarray(v) * 1e6
    return f"{np.percentile(v, 50):.1f} / {np.percentile(v, 99):.1f}"


lines = ["| clips moved | export p50 / p99 (us) | import p50 / p99 (us) | export + import p50 / p99 (us) | one step, B = 16 p50 / p99 (us) | "
         "prime of 10 s p50 / p99 (us) | blob bytes per clip | next hop of the moved clips equals the source's |", "|---|---|---|---|---|---|---|---|"]
for n in (1, 8):
    clips = list(range(3, 3 + n))
    # equality first: the hop after the move against the source itself, where the clips go on in place
    dst.import_state(src.export_state(clips), clips)
    same = torch.equal(torch.view_as_real(dst.step(frames[32])[0][clips]), torch.view_as_real(src.step(frames[32])[0][clips]))
    past = full[clips].contiguous()
    t = dict(exp=[], imp=[], pair=[], step=[], prime=[])
    holder = {}
    for i in range(iters + 10):
        a = timed(lambda: holder.__setitem__("s", src.export_state(clips)))
        b = timed(lambda: dst.import_state(holder["s"], clips))
        c = timed(lambda: dst.import_state(src.export_state(clips), clips))
        d = timed(lambda: src.step(frames[33 + i % 7], copy=False))
        e = timed(lambda: dst.prime(past, clips)) if i % 10 == 0 else None  # (2 ms each: every tenth iteration)
        if i >= 10:
            t["exp"].append(a); t["imp"].append(b); t["pair"].append(c); t["step"].append(d)
            if e is not None:
                t["prime"].append(e)
    lines.append(f"| {n} | {pct(t['exp'])} | {pct(t['imp'])} | {pct(t['pair'])} | {pct(t['step'])} | {pct(t['prime'])} | "
                 f"{holder['s'].blob.shape[1]} | {same} |")
    print(lines[-1], flush=True)
src.check_errors(); dst.check_errors()
text = "\n".join(lines) + "\n"
print(text)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)
