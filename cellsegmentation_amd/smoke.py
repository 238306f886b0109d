"""One tiny hot-path invocation on cuda:0 checked against the CPU oracle (used by __graft_entry__.smoke)."""
import os
import sys

import numpy as np
import torch


def run():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from cellsegmentation_amd import functional as HF
    from cellsegmentation_amd import kernels as K
    from cellsegmentation_amd import synth
    from cellsegmentation_amd.model import resnet as R
    from oracle import cellseg_oracle as orc      # checker only

    assert torch.cuda.is_available(), "smoke() needs cuda:0"
    dev = torch.device("cuda:0")
    arch, n, size = "resnet18", 4, 64
    x = synth.normalise(synth.ihc_tiles(n, size, seed=7))
    labels = torch.tensor([0, 1, 1, 0])
    # oracle (CPU fp32)
    sd = orc.empty_state_dict(arch)
    synth.fill_state_dict(sd)
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_()
    ref_loss = orc.tile_step_loss(sd, x, labels, arch)
    ref_loss.backward()
    ref_probs = orc.tile_probs(sd, x, arch)
    # HIP path, fp32 parity mode
    m = R.MILresnet18()
    msd = m.state_dict()
    synth.fill_state_dict(msd)
    m.load_state_dict(msd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("tile")
    m.set_encoder_grads(True)
    m.train()
    loss = HF.cross_entropy(m(x.to(dev), freeze_bn=True), labels.to(dev))
    loss.backward()
    m.eval()
    with torch.no_grad():
        probs = K.softmax_prob1(m(x.to(dev)))
    torch.cuda.synchronize()
    e_loss = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    e_prob = float(np.abs(probs.cpu().numpy() - ref_probs).max())
    g, rg = m.conv1.weight.grad.cpu(), sd["conv1.weight"].grad
    e_grad = float((g - rg).abs().max() / rg.abs().max())
    assert e_loss < 1e-4 and e_prob < 1e-4 and e_grad < 5e-3, (e_loss, e_prob, e_grad)
    # adaptive top-k on a 2-bag batch, bit-exact vs the oracle
    groups = np.repeat(np.arange(2), 32)
    pr = np.random.RandomState(3).rand(64).astype(np.float32)
    lab = {0: 0, 1: 3}
    kpt = np.where(groups == 0, 10, 3).astype(np.int32)
    out, cnt = K.segmented_topk(torch.from_numpy(pr).to(dev), torch.from_numpy(groups.astype(np.int32)).to(dev),
                                torch.from_numpy(kpt).to(dev), torch.tensor([0, 32, 64], device=dev), 32)
    got = out[: int(cnt.item())].cpu().numpy().tolist()
    assert got == orc.sample_indices(pr, groups, lab, 1, 10).tolist()
    # blended stitch: two overlapping 8x8 patches, the second given flipped horizontally with its code, against the integer formula
    from cellsegmentation_amd import detect as D
    logits = torch.randn((2, 2, 8, 8), generator=torch.Generator().manual_seed(4))
    corners = [(0, 0), (3, 5)]
    got = D.stitch_blend(logits.to(dev), corners, (12, 14), flips=[0, 1]).cpu()
    p = K.softmax_channel_fwd(logits.to(dev), 1).cpu()
    q = (256.0 * (255.0 * p).clamp(0, 255)).to(torch.int64)
    q[1] = q[1].flip(-1)                                                    # back to where its pixels lie on the slide
    t = torch.from_numpy(D.blend_taps(8).astype(np.int64))
    w = t[:, None] * t[None, :]
    num, den = torch.zeros((12, 14), dtype=torch.int64), torch.zeros((12, 14), dtype=torch.int64)
    for b, (r, c) in enumerate(corners):
        num[r:r + 8, c:c + 8] += w * q[b]
        den[r:r + 8, c:c + 8] += w
    want = torch.where(den > 0, num // (256 * den.clamp(min=1)), 0).to(torch.uint8)
    assert torch.equal(got, want) and int(got[3:8, 5:8].max()) > 0, "blended stitch differs from the integer formula"
    # bf16 throughput mode runs
    m.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        m(x.to(dev))
    torch.cuda.synchronize()
    print(f"smoke ok: loss rel err {e_loss:.2e}, prob abs err {e_prob:.2e}, conv1 grad rel err {e_grad:.2e}, top-k exact, blend exact")
