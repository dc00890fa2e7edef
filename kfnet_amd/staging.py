"""What the classes that feed training batches to the device share (SCoordNetTrainer, Augmenter, DepthLabeler) and the two
command lines above them: the rule for an image size, the stream the launches go to, and the copy of a host or device batch
into a device buffer.  A leaf module: torch is imported where it is used, nothing else of the project is."""
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
