"""plain-torch CPU restatement of the reference's image transform (`main.py:26-36`, `data_loader.py:29-32`): ToTensor, crop,
horizontal flip, Normalize -- what the tests compare `sat_image_augment_u8` / `ImageTransform` with, bit for bit."""
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def augment(u8, params, crop, mean=MEAN, std=STD, order=None):
    """u8 uint8 [Bsrc,Hs,Ws,3] (CPU); params int [B,3] of (top, left, flip); crop (Hc, Wc); order: output b comes from
    u8[order[b]] (None: b).  Returns f32 [B,3,Hc,Wc]."""
    hc, wc = crop
    x = u8.permute(0, 3, 1, 2).float().div(255)                       # ToTensor
    rows = []
    for b, (top, left, flip) in enumerate(torch.as_tensor(params).tolist()):
        im = x[b if order is None else int(order[b]), :, top:top + hc, left:left + wc]     # RandomCrop / CenterCrop
        rows.append(im.flip(-1) if flip else im)                      # RandomHorizontalFlip
    out = torch.stack(rows).contiguous()
    m = torch.as_tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return out.sub_(m).div_(s)                                        # Normalize


def source(B, Hs, Ws, seed=0):
    """seeded uint8 [B,Hs,Ws,3] test images with the extreme values 0 and 255 forced in all over"""
    u8 = torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    flat = u8.view(-1)
    flat[0::17] = 0
    flat[5::17] = 255
    return u8
