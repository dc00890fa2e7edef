"""What the classes that feed training batches to the device share (the trainers, Augmenter, DepthLabeler) and the command
lines above them: the rule for an image size, the stream the launches go to, the copy of a host or device batch into a
device buffer, and the labels' copy.  A leaf module: torch is imported where it is used, nothing else of the project is."""
import numpy as np


def check_size(height, width, what):
    """ValueError unless height and width are positive multiples of 8: SCoordNet's three stride-2 layers put the labels the
    loss reads at every eighth pixel.  `what` names the two numbers in the message."""
    if height <= 0 or width <= 0 or height % 8 or width % 8:
        raise ValueError('%s must be positive multiples of 8, got %dx%d' % (what, height, width))


def current_stream(device):
    """The handle of torch's current stream on `device`, as the library's entry points take it."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def stage(dst, src, dtype, shape, name):
    """Copies `src`, a numpy array or a tensor on either side, into the device tensor `dst` without blocking.  ValueError,
    naming `name`, unless src has `shape` and `dtype`."""
    import torch
    if not torch.is_tensor(src):
        src = torch.from_numpy(np.ascontiguousarray(src))
    if tuple(src.shape) != tuple(shape) or src.dtype != dtype:
        raise ValueError('%s must be %s %s, got %s %s' % (name, str(dtype).replace('torch.', ''), list(shape),
                                                         str(src.dtype).replace('torch.', ''), list(src.shape)))
    dst.copy_(src, non_blocking=True)


def stage_labels(buf, labels, batch, image_size, grid, device):
    """Copies a batch's labels, a numpy array or a tensor, full-resolution [B,H,W,4] or grid-sized [B,h,w,4], into a float32
    buffer on `device` without blocking: their shape picks the stride, so the copy is torch's own.  `buf` is the buffer of
    the call before (None at first), reused when the shape repeats.  Returns (the buffer, the stride at which the loss
    reads it: 8 or 1)."""
    import torch
    B, (H, Wd), (h, w) = batch, image_size, grid
    lb = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32))
    if tuple(lb.shape) not in ((B, H, Wd, 4), (B, h, w, 4)):
        raise ValueError('labels must be float32 [%d,%d,%d,4] or grid-sized [%d,%d,%d,4], got %s'
                         % (B, H, Wd, B, h, w, tuple(lb.shape)))
    if buf is None or buf.shape != lb.shape:
        buf = torch.zeros(tuple(lb.shape), dtype=torch.float32, device=device)
    buf.copy_(lb.to(torch.float32), non_blocking=True)
    return buf, (8 if tuple(lb.shape) == (B, H, Wd, 4) else 1)
