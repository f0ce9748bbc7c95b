"""Host-side mirror of the parts of the reference's `utils/tools.py` that sit on the hot path.

Same names and call signatures as `/root/reference/utils/tools.py` (class `tools` used as a
namespace), so code written against the reference (`tools.torch_warp(x, flo)`,
`tools.occ_check_model(...)(flow_f=..., flow_b=...)`, `tools.abstract_config`, `net.load_model(...)`)
keeps working; the arithmetic runs in the HIP kernels of libupflow_hip.so.
File formats (.flo, KITTI flow PNG) live in utils/flow_io.py, the KITTI readers and the evaluation bench in
dataset/kitti_dataset.py.  Out of scope: data prefetcher, SP_transform, visualisations other than
flow_to_image and the error map (lib_to_show_flow.flow_error_image_np; its arrows, point_vec, are not built).
"""
import torch
import torch.nn as nn

from .. import ops


class tools():
    # ------------------------------------------------------------------------------------------
    class abstract_config():
        """Attribute-bag configuration (utils/tools.py:32-105): defaults are set in __init__,
        `update(dict)` overrides only attributes that already exist, `get_name()` builds a tag."""
        name_filter_out_list = []

        def _public(self):
            return {k: getattr(self, k) for k in dir(self)
                    if not k.startswith('_') and not callable(getattr(self, k)) and k != 'name_filter_out_list'}

        def get_dict(self):
            return self._public()

        def update(self, data: dict, verbose=True):
            for k in self._public():
                if k in data:
                    setattr(self, k, data[k])
                    if verbose:
                        print('set param ====  %s:   %s' % (k, data[k]))

        def get_name(self, print_now=True):
            items = sorted((k, v) for k, v in self._public().items() if k not in self.name_filter_out_list)
            if print_now:
                print('=' * 10 + '\n{')
                for k, v in items:
                    print("\t%-50s: '%s,'," % ("'%s'" % k, v))
                print('}\n' + '=' * 10)
            return ''.join('%s|%s_' % kv for kv in items)

        def update_ex_name(self, ex_name: str):
            return ex_name

        @classmethod
        def check_length_of_file_name(cls, file_name):
            return len(file_name) < 255

        @classmethod
        def check_length_of_file_path(cls, filepath):
            return len(filepath) < 4096

    # ------------------------------------------------------------------------------------------
    class abstract_model(nn.Module):
        """state_dict-only checkpointing, utils/tools.py:107-155."""

        def save_model(self, save_path):
            torch.save(self.state_dict(), save_path)

        def load_model(self, load_path, if_relax=False, if_print=True):
            if if_print:
                print('loading protrained model from %s' % load_path)
            loaded = torch.load(load_path, map_location='cpu')
            if if_relax:
                # keep only keys that exist here with the same shape (utils/tools.py:115-125)
                own = self.state_dict()
                own.update({k: v for k, v in loaded.items() if k in own and v.shape == own[k].shape})
                loaded = own
            self.load_state_dict(loaded)

        def invalidate_packed(self):
            """Drop every packed-weight copy the 16-bit convolution path keeps (model/pwc_modules.py:_PackedConv3x3).
            Needed only after in-place parameter edits that bypass autograd's version counter (`p.data.copy_()`, EMA)."""
            from ..model.pwc_modules import packed_convs
            for pc in packed_convs(self):                # (incl. the channel-octet forms, `_packed8`)
                pc.invalidate()

        def load_state_dict(self, *args, **kwargs):
            r = super().load_state_dict(*args, **kwargs)
            self.invalidate_packed()
            return r

        @classmethod
        def choose_gpu(cls, model, gpu_opt=None):
            """The reference wraps in nn.DataParallel over all GPUs (utils/tools.py:130-148).  Here the
            multi-GPU form is one process per GPU: under torch.distributed the model is wrapped in
            DistributedDataParallel on this rank's device (RCCL all-reduce), otherwise it is moved to
            one GPU."""
            import torch.distributed as dist
            if gpu_opt is None:
                if dist.is_available() and dist.is_initialized():
                    from ..parallel import ddp_wrap
                    return ddp_wrap(model)
                return model.cuda()
            if type(gpu_opt) != int:
                raise ValueError('wrong gpu config, it show be int:  %s' % (str(gpu_opt)))
            torch.cuda.set_device(gpu_opt)
            return model.cuda(gpu_opt)

        @classmethod
        def save_model_gpu(cls, model, path):
            inner = getattr(model, 'module', model)      # unwrap DDP / DataParallel (utils/tools.py:150-155)
            inner.save_model(path)

    class AverageMeter():
        """utils/tools.py:282-297."""

        def __init__(self):
            self.reset()

        def reset(self):
            self.val = 0
            self.avg = 0
            self.sum = 0
            self.count = 0

        def update(self, val, num):
            self.val = val
            self.sum += val * num
            self.count += num
            self.avg = self.sum / self.count

    class time_clock():
        """Wall-clock stopwatch (utils/tools.py time_clock)."""

        def __init__(self):
            self.st = 0.0
            self.en = 0.0

        def start(self):
            import time
            self.st = time.time()

        def end(self):
            import time
            self.en = time.time()

        def get_during(self):
            return self.en - self.st

    # ---- file formats of the data / evaluation edge (utils/tools.py:1482-1632), see utils/flow_io.py ---------------
    @classmethod
    def write_flo(cls, flow, filename):
        from . import flow_io
        flow_io.write_flo(flow, filename)

    write_flow = write_flo

    @classmethod
    def read_flo(cls, filename):
        from . import flow_io
        return flow_io.read_flo(filename)

    read_flow = read_flo

    @classmethod
    def write_kitti_png_file(cls, flow_fn, flow_data, mask_data=None):
        from . import flow_io
        flow_io.write_kitti_png_file(flow_fn, flow_data, mask_data)

    @classmethod
    def write_flow_png(cls, filename, uv, v=None, mask=None):
        from . import flow_io
        flow_io.write_flow_png(filename, uv, v, mask)

    # ---- visualisation (utils/tools.py:1342-1480); the device form is ops.flow_export(color=True) -------------------------------
    @classmethod
    def color_wheel(cls):
        """The 55-entry Middlebury colour wheel, float64 [55,3]: red -> yellow -> green -> cyan -> blue -> magenta -> red in
        segments of 15, 6, 4, 11, 13 and 6 entries, the moving channel a ramp floor(255 * i / n)."""
        import numpy as np
        wheel = np.zeros((55, 3))
        at = 0
        # (segment length, channel held at 255, channel that moves, +1 rising / -1 falling)
        for n, held, moving, sign in ((15, 0, 1, 1), (6, 1, 0, -1), (4, 1, 2, 1), (11, 2, 1, -1), (13, 2, 0, 1), (6, 0, 2, -1)):
            ramp = np.floor(255 * np.arange(n) / n)
            wheel[at:at + n, held] = 255
            wheel[at:at + n, moving] = ramp if sign > 0 else 255 - ramp
            at += n
        return wheel

    @classmethod
    def flow_to_image(cls, flow, display=False, max_rad=None):
        """flow [H,W,2] -> Middlebury colour code, uint8 [H,W,3] (utils/tools.py:1342-1480; DESIGN §12 has the arithmetic).  The
        largest radius is taken in the frame's own type (fp32 for a float32 frame), everything after it in float64, as the
        reference evaluates.  Pixels with |u| or |v| > 1e7 are unknown: black, and (0,0) for the maximum.  Two differences: the
        input is not modified, and a NaN pixel is black and left out of the maximum (the reference's scale becomes -1 for the whole
        frame).  max_rad (not in the reference): a given scale in px instead of the frame's own."""
        import numpy as np
        flow = np.asarray(flow)
        if not np.issubdtype(flow.dtype, np.floating):
            flow = flow.astype(np.float64)
        u, v = flow[:, :, 0], flow[:, :, 1]
        with np.errstate(invalid='ignore', over='ignore'):
            black = (np.abs(u) > 1e7) | (np.abs(v) > 1e7) | np.isnan(u) | np.isnan(v)
            u, v = np.where(black, 0, u).astype(flow.dtype), np.where(black, 0, v).astype(flow.dtype)
            maxrad = np.max(np.sqrt(u * u + v * v)) if max_rad is None or not max_rad > 0 else np.float32(max_rad)
            if display:
                print("max flow: %.4f\nflow range:\nu = %.3f .. %.3f\nv = %.3f .. %.3f" % (maxrad, u.min(), u.max(), v.min(), v.max()))
            d = np.float64(maxrad) + np.finfo(np.float64).eps
            u, v = u.astype(np.float64) / d, v.astype(np.float64) / d
            rad = np.sqrt(u * u + v * v)
            fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54 + 1
            k0 = np.floor(fk).astype(np.int64)
            k1 = np.where(k0 + 1 == 56, 1, k0 + 1)
            f = fk - k0
            wheel = cls.color_wheel()
            img = np.zeros(u.shape + (3,), dtype=np.uint8)
            for i in range(3):
                col = (1 - f) * (wheel[k0 - 1, i] / 255) + f * (wheel[k1 - 1, i] / 255)
                col = np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
                img[:, :, i] = np.where(black, 0, np.floor(255 * col)).astype(np.uint8)
        return img

    class lib_to_show_flow():
        """The part of the reference's tools.lib_to_show_flow that an evaluation run uses (utils/tools.py:702-758); the device form
        is ops.flow_error_image.  point_vec (arrows drawn with cv2) is out of scope."""
        # the KITTI devkit's log colour map: error in [lower, upper) -> R, G, B
        ERROR_COLORS = ((0, 0.0625, 49, 54, 149), (0.0625, 0.125, 69, 117, 180), (0.125, 0.25, 116, 173, 209),
                        (0.25, 0.5, 171, 217, 233), (0.5, 1, 224, 243, 248), (1, 2, 254, 224, 144), (2, 4, 253, 174, 97),
                        (4, 8, 244, 109, 67), (8, 16, 215, 48, 39), (16, 1e9, 165, 0, 38))

        @classmethod
        def flow_error_image_np(cls, flow_pred, flow_gt, mask_occ, mask_noc=None, log_colors=True):
            """The end-point error of flow_pred against flow_gt (both [H,W,2]) as a colour image, float [H,W,3] in 0..1 with the
            channels in B, G, R order, as the reference returns it.  mask_occ [H,W,1]: 1 at every pixel with ground truth;
            mask_noc [H,W,1]: 1 where that pixel is not occluded (None: everywhere).
            log_colors: the devkit's map of min(error / 3, 20 * error / |gt|) — the outlier criterion, 1 at its threshold — in ten
            bins; occluded pixels at half brightness, pixels without ground truth black, as is an error no bin holds (NaN, inf,
            1e9 and above).  Else: min(error, 5) / 5 as brightness, red where occluded.  The table is kept as float32(c / 255),
            as the reference keeps it, so that 255 * image rounds to the same bytes."""
            import numpy as np
            if mask_noc is None:
                mask_noc = np.ones(mask_occ.shape)
            with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
                diff = np.sqrt(np.sum((flow_pred - flow_gt) ** 2, axis=2, keepdims=True))
                if not log_colors:
                    level = (np.minimum(diff, 5) / 5) * mask_occ
                    seen = level * mask_noc
                    return np.concatenate([seen, seen, level], axis=2)                     # B, G, R
                table = np.asarray(cls.ERROR_COLORS, dtype=np.float32)
                table[:, 2:] = table[:, 2:] / 255
                mag = np.sqrt(np.sum(np.square(flow_gt), axis=2, keepdims=True))
                err = np.minimum(diff / 3, 20 * diff / (mag + 1e-7))
                im = np.zeros(err.shape[:2] + (3,))
                for row in table:
                    inside = np.logical_and(err >= row[0], err < row[1])                   # [H,W,1]: broadcasts over the channels
                    im = np.where(inside, row[2:].astype(np.float64), im)
                im = np.where(mask_noc == 1, im, im * 0.5)
                im = im * mask_occ
            return im[:, :, ::-1]

    @classmethod
    def flow_error_image_u8(cls, flow_pred, flow_gt, mask_occ, mask_noc=None, log_colors=True):
        """lib_to_show_flow.flow_error_image_np as the bytes of an 8-bit RGB image, uint8 [H,W,3] in R, G, B order:
        rint(255 * image) in float64, a NaN as 0 — what ops.flow_error_image renders on the device, so that host and device write
        the same file (flow_io.write_png takes it as it is)."""
        import numpy as np
        im = cls.lib_to_show_flow.flow_error_image_np(flow_pred, flow_gt, mask_occ, mask_noc, log_colors)
        with np.errstate(invalid='ignore'):
            x = np.rint(255.0 * im[:, :, ::-1].astype(np.float64))
            return np.where(np.isnan(x), 0.0, x).astype(np.uint8)

    class abs_test_model():
        """Evaluation protocol of utils/tools.py:157-164."""
        save_dir = ''

        def eval_forward(self, im1, im2, gt, *args):
            return 0

        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            pass

    # ------------------------------------------------------------------------------------------
    class boundary_dilated_warp():
        """Photometric-loss warp that samples the UN-cropped image, so flow leaving the crop still finds
        pixels (utils/tools.py:351-499).  Clamp-to-edge bilinear gather: indices are clamped to the
        image and the weights are computed from the CLAMPED corner coordinates (:409-412, :458-466).
        One HIP gather launch (csrc/loss.hip: upf_boundary_warp_*), differentiable wrt the flow."""

        @classmethod
        def warp_im(cls, I_nchw, flow_nchw, start_n211):
            return ops.boundary_warp(I_nchw, flow_nchw, start_n211)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def torch_warp(cls, x, flo):
        """Backward warp without validity mask (utils/tools.py:1274-1319) — one HIP launch."""
        return ops.warp(x, flo, None)

    @classmethod
    def torch_warp_mask(cls, x, flo):
        """utils/tools.py:1229-1272: warp, and a mask with `mask < 0.9999 -> 0, else 1`.
        The reference thresholds grid_sample(ones) at 0.9999 here (not >= 1.0); that sum is a smooth
        function of the position, so it is evaluated from the warped ones tensor."""
        out = ops.warp(x, flo, None)
        m = ops.warp(torch.ones_like(x), flo, None)
        m = (m >= 0.9999).to(out.dtype)
        return out * m, m

    @classmethod
    def check_tensor(cls, data, name, print_data=False, print_in_txt=None):
        if data.is_cuda:
            data = data.detach().cpu()
        a = data.float().numpy()
        print(name, a.shape, 'max', a.max(), 'min', a.min(), 'mean', a.mean())

    # ------------------------------------------------------------------------------------------
    class occ_check_model():
        """Forward-backward consistency occlusion masks (utils/tools.py:501-677).
        `obj_out_all`: 'all' = consistency check only, 'out' = outgoing-flow mask only,
        'obj' = consistent OR leaving the image (the configuration model/upflow.py:364-365 uses)."""

        def __init__(self, occ_type='for_back_check', occ_alpha_1=1.0, occ_alpha_2=0.05, sum_abs_or_squar=True, obj_out_all='all'):
            self.occ_type_ls = ['for_back_check', 'forward_warp']
            assert occ_type in self.occ_type_ls
            assert obj_out_all in ['obj', 'out', 'all']
            self.occ_type = occ_type
            self.occ_alpha_1 = occ_alpha_1
            self.occ_alpha_2 = occ_alpha_2
            self.sum_abs_or_squar = True
            self.obj_out_all = obj_out_all

        def __call__(self, flow_f, flow_b, scale=1):
            if self.occ_type != 'for_back_check':
                raise ValueError('not implemented')
            if self.obj_out_all == 'obj':
                # fused kernel: 2 warps + magnitudes + thresholds + outgoing mask in one launch
                return ops.occ_check(flow_f, flow_b, self.occ_alpha_1, self.occ_alpha_2 / scale)
            if self.obj_out_all == 'all':
                return self._forward_backward_occ_check(flow_f, flow_b, scale)
            return self.torch_outgoing_occ_check(flow_f), self.torch_outgoing_occ_check(flow_b)

        def _forward_backward_occ_check(self, flow_fw, flow_bw, scale=1):
            def mag(v):                                    # utils/tools.py:559: sum_c sqrt(v_c^2)
                return v.abs().sum(dim=1, keepdim=True)
            m = mag(flow_fw) + mag(flow_bw)
            bw_w = tools.torch_warp(flow_bw, flow_fw)
            fw_w = tools.torch_warp(flow_fw, flow_bw)
            thr = self.occ_alpha_1 * m + self.occ_alpha_2 / scale
            return (mag(flow_fw + bw_w) < thr).float(), (mag(flow_bw + fw_w) < thr).float()

        @classmethod
        def torch_outgoing_occ_check(cls, flow):
            B, C, H, W = flow.shape
            xx = torch.arange(W, device=flow.device, dtype=torch.float32).view(1, 1, 1, W)
            yy = torch.arange(H, device=flow.device, dtype=torch.float32).view(1, 1, H, 1)
            px = xx + flow[:, 0:1].float()
            py = yy + flow[:, 1:2].float()
            return ((px <= W - 1) & (px >= 0) & (py <= H - 1) & (py >= 0)).float()

        @classmethod
        def torch_get_obj_occ_check(cls, occ_mask, out_occ):
            return ((occ_mask == 1) | (out_occ == 0)).to(occ_mask.dtype)
