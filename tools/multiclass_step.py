"""K = 80 R101 480x480 B = 32 bf16 detection training steps (forward, multi-class focal loss, backward) and the class maximum over
the step's classification, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -o mc -- python tools/multiclass_step.py
(profiles/r07_multiclass_k80.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from multiposenet.pytorch_amd import ops, synthetic as weightgen  # noqa: E402
from multiposenet.pytorch_amd.network.posenet import poseNet  # noqa: E402

K, B, S = 80, 32, 480
m = poseNet(101, compute_dtype=torch.bfloat16, num_classes=K).cuda()
shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
sd = weightgen.gen_state_dict(shapes, seed=0, flavour="he", skip_prefixes=("prn.",))
m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
for p in m.prn.parameters():
    p.requires_grad = False
m.train()
img = torch.from_numpy(weightgen.gen_images(1, B, S, S)).cuda()
anno = weightgen.gen_boxes_gt(2, B, S)
for b in range(B):
    for i in range(anno.shape[1]):
        if anno[b, i, 4] != -1:
            anno[b, i, 4] = float((b + 3 * i) % K)
anno = torch.from_numpy(anno).cuda()
for it in range(3):
    m.zero_grad()
    _, saved = m([img, "detection_subnet"])
    loss, log = poseNet.build_loss(saved, "detection_subnet", anno)
    loss.backward()
    cls = saved[0].detach()
    for _ in range(3):
        score, cid = ops.class_max(cls)
    torch.cuda.synchronize()
    print("step %d loss %.4f cls %s" % (it, float(loss), tuple(cls.shape)), flush=True)
print("done")
