"""The brain-extraction step of the reference's README ([B], notebooks/[B] Brain Extraction.ipynb) as two calls: load the
extractor's checkpoint, and turn volumes into cleaned brain masks on the GPU."""
import torch

NOTEBOOK_ENC_NF = (4, 8, 16, 32)
NOTEBOOK_DEC_NF = (32, 16, 8, 4)


def load_brain_extractor(path, enc_nf=NOTEBOOK_ENC_NF, dec_nf=NOTEBOOK_DEC_NF, use_in=False):
    """Simple_Unet(1, 1, ...) with the weights of the reference's checkpoint layout: torch.load(path)["u1"], keys with or
    without the "module." prefix nn.DataParallel adds (the notebook saves the wrapped model), loaded with strict=True.
    Returned on the CPU in eval mode."""
    from ..model import Simple_Unet
    state = torch.load(path, map_location="cpu", weights_only=False)["u1"]
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    net = Simple_Unet(1, 1, use_in, list(enc_nf), list(dec_nf))
    net.load_state_dict(state, strict=True)
    return net.eval()


def extract_brain(net, img, size=(128, 128, 128), level=0.5, clean_threshold=0.2):
    """The notebook's prediction cell for img (N, 1, D, H, W) on the GPU: trilinear resize to `size`, `net` under no_grad, x2
    trilinear upsampling, threshold with >= level, clean_mask per sample -> (N, 2 size) uint8 masks on the GPU.  (The notebook's
    permutes belong to its loader's orientation and are left out.)"""
    from .. import ops
    from ..utils import resize_trilinear
    if img.dim() != 5 or img.shape[1] != 1:
        raise ValueError(f"extract_brain: expected (N, 1, D, H, W), got {tuple(img.shape)}")
    with torch.no_grad():
        x = resize_trilinear(img, size=tuple(size))
        prob = resize_trilinear(net(x), scale_factor=2)
        mask = (prob[:, 0] >= level).to(torch.uint8)
        out, info = ops.clean_mask3d(mask, clean_threshold)
    if 0 in info[:-1].tolist():
        raise ValueError("extract_brain: a predicted mask is empty (no voxel reaches the level)")
    return out
