"""The volume shape entry on a batch that lies in device memory (tests/test_volshape_gpu.py)."""
import numpy as np

from nyxus_amd import _abi, _lib


def device_rows(ctx, b, s, smask=_abi.VSHAPE_MORPHOLOGY, stated=True, max_device_bytes=0):
    """The table of HostBatch3D `b` through nyxhip_featurize_volumes_shape with every array copied to cuda:0 first and the table written
    on the device (two guard columns behind the row stay untouched)."""
    import torch
    dev = torch.device("cuda", 0)
    view = {2: np.int16, 4: np.int32, 8: np.int64}
    keep = {k: torch.from_numpy(getattr(b, k).view(view[getattr(b, k).dtype.itemsize])).to(dev)
            for k in ("px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")}
    h = b.c_struct(stated=stated, max_device_bytes=max_device_bytes)
    cb = _abi.Batch3D()
    cb.n_roi = b.n_roi
    for k, v in keep.items():
        setattr(cb, k, v.data_ptr())
    cb.memory = _abi.MEM_DEVICE
    cb.max_px, cb.max_bbox_cells, cb.max_inten_range, cb.max_device_bytes = h.max_px, h.max_bbox_cells, h.max_inten_range, h.max_device_bytes
    ncol = len(_lib.volshape_column_names(smask))
    ld = ncol + 2
    out = torch.full((b.n_roi, ld), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.volumes_shape_device(cb, smask, s, out.data_ptr(), ld)
    G = out.cpu().numpy()
    assert (G[:, ncol:] == -1.0).all()
    return np.ascontiguousarray(G[:, :ncol])
