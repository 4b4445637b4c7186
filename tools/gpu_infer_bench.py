"""Inference throughput: whole-image forward + on-GPU top-K decode + NMS (BASELINE.json: fps at 512x512; config 5: 1920x1080).
Single-image detect() rows and batched detect_batch() rows (one forward + one decode / NMS launch per call), timed in the same
process.  Every row is warmed (graph capture included), then timed over >= 0.5 s with a host clock: each call ends in a stream
sync (the results are on the host).  TFLOP/s is END-TO-END: the network's algorithmic FLOP / the whole call's wall time (host
work, input copy, decode, result copies included), not a kernel's share of MFMA peak.
usage: python tools/gpu_infer_bench.py [kind] [dtype]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import densebox_amd as D
from densebox_amd import synth
kind = sys.argv[1] if len(sys.argv) > 1 else 'DenseBox'
dtype = sys.argv[2] if len(sys.argv) > 2 else 'f16'
net = getattr(D, kind)(synth.vgg19_standin(0)); synth.fill_params_(net, 11); net = net.cuda().eval(); net.compute_dtype = dtype
GF240 = {'DenseBox': 41.98, 'DenseBoxLM': 44.95, 'DenseBoxLMLOC': 47.81}[kind]
ROWS = [(512, 512, 1, 10), (512, 512, 8, 10), (512, 512, 32, 10), (512, 512, 64, 10),
        (1080, 1920, 1, 10), (1080, 1920, 1, 1000), (1080, 1920, 4, 10), (1080, 1920, 8, 10)]
for (h, w, n, K) in ROWS:
    x = synth.synth_images(n, h, w, seed=1).cuda()
    if n == 1:
        def run():
            return net.detect(x, K=K, nms_thresh=0.4)
        what = 'detect()       forward+topK(%d)+NMS' % K
    else:
        def run():
            return net.detect_batch(x, K=K, nms_thresh=0.4, max_batch=n)
        what = 'detect_batch() forward+topK(%d)+NMS, B=%d' % (K, n)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    run()                                            # first call: warm-up forwards + graph capture
    torch.cuda.synchronize()
    m1 = torch.cuda.memory_allocated()
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    it, t0 = 0, time.perf_counter()
    while True:
        run()                                        # (ends in a stream sync: results on the host)
        it += 1
        dt = time.perf_counter() - t0
        if dt >= 0.5 and it >= 10:
            break
    dt /= it
    gf = GF240 * (h * w) / (240 * 240) * n
    print('%s %s %4dx%-4d %-44s %8.3f ms/call  %7.1f img/s  %6.1f TFLOP/s end-to-end  (%d calls; first call +%.1f MiB device memory)'
          % (kind, dtype, w, h, what, dt * 1e3, n / dt, gf / dt / 1e3, it, (m1 - m0) / 2**20), flush=True)
