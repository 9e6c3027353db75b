"""Dataset preparation on the device -- the reference's offline notebooks
(notebooks/calculating_diversity_for_data.ipynb, calculate_and_analysis_of_max_coordinates.ipynb,
data_filtering.ipynb) as two HIP kernels (csrc/prepare.hip) and the frames around them.

The ``pickle`` data source (data_transformations.py) needs four things the detector simulation does not
write.  With x the stored, log1p-domain images [N,H,W] and c the [N,9] float64 matrix of COND_COLUMNS:

* ``group_number[i]``  rank of row c[i] among the distinct rows of c in lexicographic order
  (``np.unique(c, axis=0, return_inverse=True)[1]`` = ``DataFrame.groupby(COND_COLUMNS).ngroup()``);
* ``std[i]`` (``std_proton``)  the SDI-GAN diversity: per group and pixel the population standard
  deviation (ddof = 0, fp64) over the group's images, summed over the pixels (``group_sum``), divided by
  the largest group_sum;
* ``neutron_photon_sum`` / ``proton_photon_sum``  ``np.sum(x[i])`` in fp64;
* ``max_x, max_y``  ``np.unravel_index(np.argmax(x[i]), (H, W))``: row and column of the first maximum.

The one deliberate difference from the notebooks: when every group has a single member every group_sum
is 0 and pandas gives 0/0 = NaN; `diversity` returns zeros and logs a warning.

The proton sets' ``expert_number`` column is a clustering of the images: `prepare_dataset(n_clusters=K)` computes
it on the device (utils/clustering.py: k-means of the filtered images, clusters numbered from the faintest).
Without n_clusters it keeps an ``expert_number`` column the frame already has (or takes one as an argument) and
otherwise writes zeros, one cluster, with a warning.

There is no CPU fallback: without a HIP device every device function raises (hip.HipError).
Only load pickles you produced yourself: unpickling executes code from the file.
"""
from __future__ import annotations

import ctypes as C
import logging
import os

import numpy as np
import torch

from .. import hip
from ..segments import is_f64, work_buffer
from .data_transformations import COND_COLUMNS, ZDCType, _photon_sum_column

logger = logging.getLogger(__name__)

FILE_NAMES = {"DATA_IMAGES_PATH": "data_{zdc}.pkl", "DATA_COND_PATH": "data_cond_{zdc}.pkl",
              "DATA_POSITIONS_PATH": "data_coord_{zdc}.pkl"}


# ---------------------------------------------------------------------------------------------
# host side: groups
# ---------------------------------------------------------------------------------------------

def group_numbers(cond):
    """cond [N,9] (array or the COND_COLUMNS of a frame) -> (group int64 [N], n_groups): the rank of each
    row among the distinct rows in lexicographic order.  Host, numpy.  Raises ValueError on a non-finite
    condition."""
    c = np.ascontiguousarray(np.asarray(cond, dtype=np.float64))
    if c.ndim != 2:
        raise ValueError(f"conditions must be [N, columns], got {c.shape}")
    bad = ~np.isfinite(c)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise ValueError(f"non-finite condition at row {i}, column {j}")
    if c.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), 0
    uniq, inverse = np.unique(c, axis=0, return_inverse=True)
    return inverse.reshape(-1).astype(np.int64), int(uniq.shape[0])


def _device(device=None):
    if not torch.cuda.is_available():
        raise hip.HipError("dataset preparation needs a HIP device (no CPU fallback)")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def group_layout(group, n_groups: int, device=None):
    """(perm int32 [N], offs int32 [n_groups + 1]) on the device, es_router_dispatch's layout: the members of
    group g are perm[offs[g] .. offs[g+1]), in ascending sample index."""
    dev = _device(device)
    g = torch.as_tensor(np.asarray(group) if not isinstance(group, torch.Tensor) else group).to(dev, torch.int64)
    perm = torch.argsort(g, stable=True).to(torch.int32)
    counts = torch.bincount(g, minlength=int(n_groups))[:int(n_groups)]
    offs = torch.zeros(int(n_groups) + 1, dtype=torch.int32, device=dev)
    offs[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return perm, offs


# ---------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------

def _as_device_images(images, device=None) -> torch.Tensor:
    """[N,H,W] fp32 or fp64 on the device, any strides (host data is copied; other dtypes widen to fp64)."""
    t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError(f"images must be [N,H,W], got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if t.shape[1] * t.shape[2] < 1 or t.shape[1] * t.shape[2] > 4096:
        raise ValueError(f"images of {t.shape[1]}x{t.shape[2]} are outside 1 <= H*W <= 4096")
    if not t.is_cuda:
        t = t.to(_device(device), non_blocking=True)
    return t


def _view(x):
    N, H, W = x.shape
    return hip.make_view((N, 1, H, W), (x.stride(0), H * W, x.stride(1), x.stride(2)), False)


def _first_bad_image(x) -> int:
    bad = ~torch.isfinite(x).flatten(1).all(dim=1)
    return int(torch.nonzero(bad)[0])


def diversity_raw(x, perm, offs, n_groups: int, return_maps: bool = False):
    """es_group_diversity on device tensors: (group_sum [G] fp64, pix_var [G, H*W] fp64 or None).  No host
    synchronisation; runs on the current stream."""
    hip.require_device(x)
    N, H, W = x.shape
    G = int(n_groups)
    group_sum = torch.zeros(G, dtype=torch.float64, device=x.device)
    pix_var = torch.zeros(G, H * W, dtype=torch.float64, device=x.device) if return_maps else None
    if N == 0 or G == 0:
        return group_sum, pix_var
    view = _view(x)
    with torch.cuda.device(x.device):
        need = int(hip.lib().es_group_diversity_workspace(G, H, W))
        work = work_buffer(need, x.device)
        hip.call("es_group_diversity", C.byref(view), is_f64(x), hip.ptr(x),
                 hip.ptr(perm), hip.ptr(offs), G, hip.ptr(group_sum), hip.ptr(pix_var), hip.ptr(work), need,
                 hip.stream_ptr())
    return group_sum, pix_var


def diversity(images, group, n_groups: int, device=None, return_maps: bool = False):
    """(std [N] fp64, group_sum [G] fp64[, pix_var [G, H*W] fp64]) device tensors: the SDI-GAN diversity of
    every sample, group_sum[group] / max(group_sum), normalised by the device maximum.  images fp32 / fp64,
    host or device.  All-singleton groups: zeros and a warning (pandas: NaN).  Raises ValueError on a
    non-finite pixel, naming the first offending image."""
    x = _as_device_images(images, device)
    perm, offs = group_layout(group, n_groups, x.device)
    group_sum, pix_var = diversity_raw(x, perm, offs, n_groups, return_maps)
    g = torch.as_tensor(np.asarray(group) if not isinstance(group, torch.Tensor) else group).to(x.device, torch.int64)
    if group_sum.numel() == 0:
        std = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
        return (std, group_sum, pix_var) if return_maps else (std, group_sum)
    top = group_sum.max()
    # the one copy out: [all finite, the maximum is positive]
    finite, positive = torch.stack([torch.isfinite(group_sum).all(), top > 0]).tolist()
    if not finite:
        raise ValueError(f"non-finite pixel in image {_first_bad_image(x)}")
    if positive:
        std = (group_sum / top)[g]
    else:
        logger.warning("diversity: every group sum is 0 (all groups have one member, or all images of a group "
                       "are identical); returning zeros where pandas gives 0/0 = NaN")
        std = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
    return (std, group_sum, pix_var) if return_maps else (std, group_sum)


def photon_sums_and_peaks(images, device=None, check: bool = True):
    """(sum [N] fp64, peak [N,2] int32) device tensors (es_image_sum_peak): np.sum of every image in fp64
    and (row, col) of its first maximum.  Raises ValueError on a non-finite pixel (check=False: no copy out
    and no check)."""
    x = _as_device_images(images, device)
    N, H, W = x.shape
    s = torch.empty(N, dtype=torch.float64, device=x.device)
    peak = torch.empty(N, 2, dtype=torch.int32, device=x.device)
    if N == 0:
        return s, peak
    view = _view(x)
    with torch.cuda.device(x.device):
        hip.call("es_image_sum_peak", C.byref(view), is_f64(x), hip.ptr(x), hip.ptr(s),
                 hip.ptr(peak), hip.stream_ptr())
    if check and not bool(torch.isfinite(s).all()):
        raise ValueError(f"non-finite pixel in image {_first_bad_image(x)}")
    return s, peak


# ---------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------

def _zdc(zdc_type) -> str:
    z = zdc_type.value if isinstance(zdc_type, ZDCType) else str(zdc_type)
    if z not in (ZDCType.PROTON.value, ZDCType.NEUTRON.value):
        raise ValueError("Unsupported ZDC type! Choose either proton or neutron.")
    return z


def photon_sum_mask(photon_sum, min_photon_sum=None, max_photon_sum=None):
    """The notebooks' filter_photon_sum for one detector: keep min <= photon_sum <= max (a bound of None is
    not applied)."""
    s = np.asarray(photon_sum, dtype=np.float64)
    keep = np.ones(s.shape[0], dtype=bool)
    if min_photon_sum is not None:
        keep &= s >= float(min_photon_sum)
    if max_photon_sum is not None:
        keep &= s <= float(max_photon_sum)
    return keep


def assemble_frames(cond_frame, zdc_type, std, group, photon_sum, peak, expert_number=None):
    """Host-side assembly: the conditions frame `get_dataset` + `transform_data_for_training` accept
    (COND_COLUMNS first, then the derived columns under the detector's names) and the positions frame.
    A neutron_photon_sum column the frame already has is kept (the simulation's own PhotonSum, as the
    notebook keeps it); proton_photon_sum is always the computed sum."""
    import pandas as pd
    zdc = _zdc(zdc_type)
    missing = [c for c in COND_COLUMNS if c not in cond_frame.columns]
    if missing:
        raise ValueError(f"the conditions frame lacks {missing}")
    ps_col = _photon_sum_column(zdc)
    out = cond_frame[COND_COLUMNS].reset_index(drop=True).copy()
    n = len(out)
    std, group, photon_sum, peak = (np.asarray(a) for a in (std, group, photon_sum, peak))
    if not (std.shape == (n,) and group.shape == (n,) and photon_sum.shape == (n,) and peak.shape == (n, 2)):
        raise ValueError("derived columns do not match the frame's length")
    if zdc == ZDCType.PROTON.value:
        out["std_proton"] = std.astype(np.float64)
        out[ps_col] = photon_sum.astype(np.float64)
        out["group_number_proton"] = group.astype(np.int64)
        if expert_number is None and "expert_number" in cond_frame.columns:
            expert_number = cond_frame["expert_number"].to_numpy()
        if expert_number is None:
            logger.warning("no expert_number given: writing zeros (prepare_dataset(n_clusters=K) clusters the images)")
            expert_number = np.zeros(n, dtype=np.int64)
        out["expert_number"] = np.asarray(expert_number)
    else:
        out["std"] = std.astype(np.float64)
        kept = cond_frame[ps_col].to_numpy() if ps_col in cond_frame.columns else None
        out[ps_col] = kept if kept is not None else photon_sum.astype(np.float64)
        out["group_number"] = group.astype(np.int64)
    positions = pd.DataFrame({"max_x": peak[:, 0].astype(np.int64), "max_y": peak[:, 1].astype(np.int64)})
    return out, positions


def prepare_dataset(images, cond_frame, zdc_type, min_photon_sum=None, max_photon_sum=None, device=None,
                    expert_number=None, n_clusters=None, cluster_seed=0, cluster_restarts=10):
    """images [N,H,W] (log1p domain, fp32 / fp64, host or device) + the particle conditions frame ->
    (images, cond_frame, positions_frame) ready for write_dataset / the ``pickle`` source.

    The photon-sum filter is applied first (on the neutron frame's own neutron_photon_sum when it has one,
    else on the computed sums), then std / group_number / photon sum are added and the positions frame is
    built.  Device copies out: the packed sums and peaks, diversity's two flags and the std column.

    n_clusters (proton sets only): ``expert_number`` = clustering.cluster_images of the filtered images into
    that many clusters (k-means++ with cluster_restarts restarts from cluster_seed).  It excludes a given
    expert_number -- the argument or a column of the frame -- and a neutron set: ValueError."""
    zdc = _zdc(zdc_type)
    ps_col = _photon_sum_column(zdc)
    cond_frame = cond_frame.reset_index(drop=True)
    if n_clusters is not None:
        if zdc != ZDCType.PROTON.value:
            raise ValueError("n_clusters: only the proton sets have an expert_number column")
        if expert_number is not None or "expert_number" in cond_frame.columns:
            raise ValueError("n_clusters together with a given expert_number: choose one")
        if int(n_clusters) < 1:
            raise ValueError(f"n_clusters = {n_clusters}")
    if len(cond_frame) != len(images):
        raise ValueError(f"{len(images)} images but {len(cond_frame)} condition rows")
    x = _as_device_images(images, device)
    sums, peak = photon_sums_and_peaks(x, check=False)
    packed = torch.cat([sums[:, None], peak.double()], dim=1).cpu().numpy()      # one copy out for both
    sums, peak = packed[:, 0].copy(), packed[:, 1:].astype(np.int32)
    if not np.isfinite(sums).all():
        raise ValueError(f"non-finite pixel in image {int(np.flatnonzero(~np.isfinite(sums))[0])}")
    own = zdc == ZDCType.NEUTRON.value and ps_col in cond_frame.columns
    filt = cond_frame[ps_col].to_numpy() if own else sums
    keep = photon_sum_mask(filt, min_photon_sum, max_photon_sum)
    if not keep.all():
        logger.info("photon-sum filter keeps %d of %d samples", int(keep.sum()), len(keep))
        idx = np.flatnonzero(keep)
        x = x[torch.from_numpy(idx).to(x.device)]
        images = images[idx] if not isinstance(images, torch.Tensor) else images[torch.from_numpy(idx).to(images.device)]
        cond_frame = cond_frame[keep].reset_index(drop=True)
        sums, peak = sums[keep], peak[keep]
        if expert_number is not None:
            expert_number = np.asarray(expert_number)[keep]
    group, n_groups = group_numbers(cond_frame[COND_COLUMNS].to_numpy(dtype=np.float64))
    std, _ = diversity(x, group, n_groups)
    if n_clusters is not None:
        from .clustering import cluster_images
        expert_number = cluster_images(x, int(n_clusters), n_init=int(cluster_restarts),
                                       seed=int(cluster_seed))[0].cpu().numpy()
    cond_out, positions = assemble_frames(cond_frame, zdc, std.cpu().numpy(), group, sums, peak, expert_number)
    host_images = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    return host_images, cond_out, positions


def dataset_paths(out_dir, zdc_type):
    """{DATA_IMAGES_PATH, DATA_COND_PATH, DATA_POSITIONS_PATH: file} under out_dir."""
    zdc = _zdc(zdc_type)
    return {k: os.path.join(str(out_dir), v.format(zdc=zdc)) for k, v in FILE_NAMES.items()}


def write_dataset(out_dir, zdc_type, images, cond_frame, positions_frame, cfg=None):
    """Write the three pickles of the ``pickle`` source under out_dir; returns {config key: path}, to be
    passed as ``dataset.DATA_*_PATH`` overrides.  With cfg the files take the base names its
    ``dataset.DATA_*_PATH`` keys point to, else FILE_NAMES."""
    import pandas as pd
    paths = dataset_paths(out_dir, zdc_type)
    if cfg is not None:
        paths = {k: os.path.join(str(out_dir), os.path.basename(str(cfg.dataset[k]))) for k in paths}
    os.makedirs(str(out_dir), exist_ok=True)
    pd.to_pickle(np.asarray(images), paths["DATA_IMAGES_PATH"])
    cond_frame.to_pickle(paths["DATA_COND_PATH"])
    positions_frame.to_pickle(paths["DATA_POSITIONS_PATH"])
    return paths
