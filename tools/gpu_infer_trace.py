"""Inference (detect(), or detect_batch() when B > 1: hipGraph replay) repeated a few times, for a rocprofv3 kernel trace.
usage: python tools/gpu_infer_trace.py [H] [W] [dtype] [B] [kind]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import densebox_amd as D
from densebox_amd import synth
h = int(sys.argv[1]) if len(sys.argv) > 1 else 512
w = int(sys.argv[2]) if len(sys.argv) > 2 else 512
dtype = sys.argv[3] if len(sys.argv) > 3 else 'f16'
n = int(sys.argv[4]) if len(sys.argv) > 4 else 1
kind = sys.argv[5] if len(sys.argv) > 5 else 'DenseBoxLMLOC'
net = getattr(D, kind)(synth.vgg19_standin(0)); synth.fill_params_(net, 11); net = net.cuda().eval(); net.compute_dtype = dtype
x = synth.synth_images(n, h, w, seed=1).cuda()
for _ in range(12):
    if n == 1:
        net.detect(x, K=10, nms_thresh=0.4)
    else:
        net.detect_batch(x, K=10, nms_thresh=0.4, max_batch=n)
torch.cuda.synchronize()
