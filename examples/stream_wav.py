#!/usr/bin/env python3
"""Real-time style enhancement of a 16 kHz mono WAV file, 8 ms at a time, on one MI355X.

    python examples/stream_wav.py noisy.wav enhanced.wav [--ckpt path/to/checkpoints/best] [--model fullsubnet|cirm|frozen]

Every 128-sample hop goes through ONE launch (sfsn_stream_hop in waveform mode: STFT of the new frame, the whole
Spiking-FullSubNet, inverse STFT with its overlap-add state); samples are read from and written to pinned host memory by the
launch itself.  --model cirm streams the cIRM-GSN baseline (modeling_cirm_gsn.Model at its recipe) the same way, through
sfsn_fullband_stream_hop_wave.  The output lags the input by 384 samples (24 ms: the look-ahead of the reference's centred 32 ms analysis plus the
overlap-add) -- the script drops that lead-in and flushes the tail with zeros, so the file lengths match.
Without --ckpt the weights are the reference's random initialisation (useful as a latency demo only).

--model frozen streams the model_zoo architecture (model_low_freq.Separator with offline_laplace_norm: baseline_m, or baseline_s with
--zoo s) -- the trained weights of --ckpt, or the zoo weights kept in tests/golden/frozen_{s,m}_zoo.npz.  Its normalisation divides
by per-clip means of the whole utterance, which a stream does not have: they come from an offline pass over the first
--calibrate SECONDS of the file (Separator.norm_stats) and are handed to the session (streaming(norm_stats=...)).  The default, the
whole file, reproduces the offline result model(wave) bit for bit; anything shorter is a modelling choice this project makes no
accuracy claim about.

--resample 3 takes a 48 kHz file and writes a 48 kHz file (384 samples per hop), --s16 hands the session the file's 16-bit samples as
they are and writes what it returns: decimation, interpolation and both format conversions run inside the same one launch
(streaming(resample=3, sample_format="s16"); --model cirm: Model.streaming_outer(resample=3, sample_format="s16")).  The filters add
95 samples at 48 kHz to the lead-in.
"""
import argparse
import os
import sys
import time
import wave

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiking_fullsubnet_amd as pkg  # noqa: E402

BASELINE_M = dict(  # recipes/intel_ndns/spiking_fullsubnet/baseline_m.toml [model.args]
    n_fft=512, hop_length=128, win_length=512, fdrc=0.5, fb_input_size=64, fb_hidden_size=320, fb_num_layers=2, fb_proj_size=64,
    fb_output_activate_function=False, sb_hidden_size=224, sb_num_layers=2, freq_cutoffs=[0, 32, 128, 256], df_orders=[5, 3, 1],
    center_freq_sizes=[4, 32, 64], neighbor_freq_sizes=[15, 15, 15], use_pre_layer_norm_fb=True, use_pre_layer_norm_sb=True, bn=True,
    shared_weights=True, sequence_model="GSN", num_spks=1)
FROZEN_S = dict(  # model_zoo/intel_ndns/spike_fsb/baseline_s/baseline_s.toml [model_g.args]
    sr=16000, fdrc=0.5, n_fft=512, fb_freqs=64, hop_length=128, win_length=512, num_freqs=256, sequence_model="GSU", fb_hidden_size=240,
    fb_output_activate_function=False, freq_cutoffs=[32, 128], sb_df_orders=[3, 1, 1], sb_num_center_freqs=[4, 32, 64],
    sb_num_neighbor_freqs=[15, 15, 15], fb_num_center_freqs=[4, 32, 64], fb_num_neighbor_freqs=[0, 0, 0], sb_hidden_size=160,
    sb_output_activate_function=False, norm_type="offline_laplace_norm", shared_weights=True, bn=True)
FROZEN_M = dict(FROZEN_S, fb_hidden_size=320, sb_hidden_size=224, sb_df_orders=[5, 3, 1])  # .../baseline_m/baseline_m.toml [model_g.args]
CIRM_GSN = dict(  # recipes/intel_ndns/cirm_gsn/default.toml [model.args]
    n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=268, num_layers=4, proj_size=257,
    output_activate_function=False, df_order=3, use_pre_layer_norm_fb=True, bn=True, shared_weights=True, sequence_model="GSN", num_spks=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("inp")
    ap.add_argument("out")
    ap.add_argument("--ckpt", default=None, help="an Accelerate checkpoint directory of the live recipe (pytorch_model.bin / model.safetensors)")
    ap.add_argument("--synops", action="store_true", help="count the spikes while streaming and print the clip's SynOPs / NeuronOPs")
    ap.add_argument("--model", choices=("fullsubnet", "cirm", "frozen"), default="fullsubnet", help="fullsubnet: Spiking-FullSubNet (baseline_m); "
                    "cirm: the cIRM-GSN baseline; frozen: the model_zoo architecture (offline_laplace_norm) with calibrated statistics")
    ap.add_argument("--zoo", choices=("s", "m"), default="m", help="--model frozen: baseline_s or baseline_m")
    ap.add_argument("--calibrate", type=float, default=None, metavar="SECONDS", help="--model frozen: take the normalisation statistics "
                    "from an offline pass over the first SECONDS of the file (default: the whole file = the offline result)")
    ap.add_argument("--resample", type=int, choices=(1, 3), default=1, help="3: the file is 48 kHz; it is decimated and the result "
                    "interpolated back inside the hop's launch")
    ap.add_argument("--s16", action="store_true", help="hand the session 16-bit PCM and take 16-bit PCM back (converted inside the launch)")
    args = ap.parse_args()
    outer = args.resample != 1 or args.s16
    rate, n = 16000 * args.resample, 128 * args.resample
    io_kw = dict(resample=args.resample, sample_format="s16" if args.s16 else "f32") if outer else {}
    if args.model == "cirm" and args.synops:
        ap.error("--synops: cIRM-GSN streaming sessions do not count spikes (count_spikes is built for --model fullsubnet only)")
    with wave.open(args.inp, "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2 and w.getframerate() == rate, f"{rate} Hz mono 16-bit PCM expected"
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16)
        x = pcm.astype(np.float32) / 32768.0
    if args.model == "cirm":
        from spiking_fullsubnet_amd.modeling_cirm_gsn import Model as CirmGsn
        model = CirmGsn(**CIRM_GSN)
    elif args.model == "frozen":
        model = pkg.Separator(**(FROZEN_S if args.zoo == "s" else FROZEN_M))
        if not args.ckpt:
            g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", f"frozen_{args.zoo}_zoo.npz"))
            model.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}, strict=True)
    else:
        model = pkg.SpikingFullSubNet(**BASELINE_M)
    if args.ckpt:
        from spiking_fullsubnet_amd.checkpoint import load_checkpoint
        load_checkpoint(model, args.ckpt)
    model = model.to("cuda").eval()
    if args.model == "cirm":
        sess = model.streaming_outer(batch=1, host_io=True, **io_kw) if outer else model.streaming(batch=1, waveform=True, host_io=True)
    elif args.model == "frozen":
        x16 = x
        if args.resample == 3:  # the statistics are the model's: taken at its own rate
            from spiking_fullsubnet_amd import spectral
            x16 = spectral.resample_down3(torch.from_numpy(x[:len(x) // 3 * 3].copy()).reshape(1, -1).to("cuda"))[0][0].cpu().numpy()
        n_cal = len(x16) if args.calibrate is None else min(len(x16), max(1024, int(args.calibrate * 16000)))
        stats = model.norm_stats(torch.from_numpy(x16[:n_cal].copy()).reshape(1, -1).to("cuda"))
        print(f"statistics from the first {n_cal / 16000:.2f} s: full-band mean {float(stats.mu_fb[0]):.6g}, "
              f"sub-band means {[round(v, 6) for v in stats.mu_sb[:, 0].tolist()]}")
        sess = model.streaming(batch=1, waveform=True, host_io=True, count_spikes=args.synops, norm_stats=stats, **io_kw)
    else:
        sess = model.streaming(batch=1, waveform=True, host_io=True, count_spikes=args.synops, **io_kw)
    lead = 3 * n + (95 if args.resample == 3 else 0)  # the 3 hops of algorithmic delay (+ the two filters' 47.5 samples each)
    n_hops = -(-(len(x) + lead) // n)
    src = pcm if args.s16 else x
    xp = np.zeros(n_hops * n, src.dtype)
    xp[:len(x)] = src
    y = np.zeros(n_hops * n, src.dtype)
    lat = []
    for c in range(n_hops):
        t0 = time.perf_counter()
        o = sess.step_wave_host(torch.from_numpy(xp[n * c:n * (c + 1)]).reshape(1, n))
        lat.append(time.perf_counter() - t0)
        y[n * c:n * (c + 1)] = o[0, 0].numpy()
    sess.check_errors()
    y = y[lead:lead + len(x)]  # drop the lead-in
    with wave.open(args.out, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((y if args.s16 else (np.clip(y, -1.0, 1.0) * 32767.0).astype(np.int16)).tobytes())
    lat = np.sort(np.asarray(lat[10:])) * 1e6
    print(f"{len(x) / rate:.2f} s of audio, {n_hops} hops: per-hop latency p50 {lat[len(lat) // 2]:.1f} us, p99 {lat[int(len(lat) * 0.99)]:.1f} us "
          f"({8000.0 / lat[len(lat) // 2]:.0f} x real time)")
    if args.synops:  # the utterance as streamed: every frame the session computed (the zero-padded tail included)
        from spiking_fullsubnet_amd import metric
        for b in range(sess.B):
            fb_b, sb_b = sess.spike_summary([b])
            print(f"clip {b}: {int(sess.clip_frames[b])} frames, SynOPs {metric.compute_synops(fb_b, sb_b, True):.6g}, "
                  f"NeuronOPs {metric.compute_neuronops(fb_b, sb_b):.6g}")


if __name__ == "__main__":
    main()
