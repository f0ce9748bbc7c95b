"""Evaluation entry point — mirror of `/root/reference/test.py`: `Test_model(pretrain_path)` with the reference's flags
(test.py:22-30), `eval_forward(im1, im2, gt, ...) -> flow_fw` (:40-47), `kitti_2015_test()` (:54-61).

What differs: the forward runs on the MI355X-native operators, and — because KITTI is evaluated at batch 1 on frames whose
size changes between sequences — through `runtime.ShapeCachedInference`: one captured hipGraph per frame size, replayed for
every further pair of that size (`graph=False` restores plain eager calls).  `dtype`: torch.float32 (the parity mode, the
reference's arithmetic within 1e-4 px), torch.float16 / torch.bfloat16 (the fast modes; README.md "which dtype")."""
import torch

from .utils.tools import tools
from .model.upflow import UPFlow_net

PARAM_DICT = {
    # use cost volume norm                                   (test.py:22-30)
    'if_norm_before_cost_volume': True,
    'norm_moments_across_channels': False,
    'norm_moments_across_images': False,
    'if_froze_pwc': False,
    'if_use_cor_pytorch': False,
    'if_sgu_upsample': True,
}


class Test_model(tools.abs_test_model):
    def __init__(self, pretrain_path='./scripts/upflow_kitti2015.pth', dtype=torch.float32, graph=True, device='cuda', net=None, streams=1,
                 save_dir=None, save=('kitti',), save_workers=4, max_rad=None, png='host', error_log_colors=True, error_dilate=0):
        """streams > 1: `Evaluation_bench` keeps that many frame pairs in flight (runtime.PipelinedEvaluation, through
        eval_forward_stream) instead of one at a time — same results, ~1.7x the pairs per second at KITTI's frame size.
        save_dir (not in the reference, whose runner saves on the host): eval_save_result writes, for every prediction, the files
        named in `save` — 'kitti' -> <save_dir>/flow/<name>.png (the 16-bit KITTI PNG), 'color' -> <save_dir>/color/<name>.png (the
        Middlebury rendering, scaled by max_rad px or by each frame's own largest flow), 'flo' -> <save_dir>/flo/<name>.flo —
        encoded on the device (ops.flow_export) and compressed and written by at most save_workers threads (result_saver.py);
        flush() / close() wait for the files.  None: eval_save_result prints the name, as the reference's.
        png='device': the PNGs are compressed on the device too (ops.png_encode; the same samples in other bytes).
        'error' in save -> <save_dir>/error/<name>.png, the KITTI devkit's error map against the ground truth (ops.flow_error_image;
        error_log_colors: its log colour map, else brightness; error_dilate = r in 0..4 spreads the sparse ground truth's pixels over
        r pixels).  It needs the uint16 ground truth, which Evaluation_bench(device_score=True) hands to a model whose
        `wants_gt_u16` is set — as it is here; everywhere else eval_save_result raises a ValueError."""
        super(Test_model, self).__init__()
        self.saver = None
        self.wants_gt_u16 = False
        if save_dir is not None:
            from .result_saver import ResultSaver
            self.save_dir = save_dir
            self.saver = ResultSaver(save_dir, save=save, workers=save_workers, max_rad=max_rad, png=png,
                                     error_log_colors=error_log_colors, error_dilate=error_dilate)
            self.wants_gt_u16 = 'error' in self.saver.save
        supplied = net is not None
        if net is None:
            net_conf = UPFlow_net.config()
            net_conf.update(PARAM_DICT, verbose=False)
            net = net_conf()
            if pretrain_path is not None:
                net.load_model(pretrain_path, if_relax=True, if_print=True)
        # a supplied network that is already 16-bit — possibly MIXED (UPFlow_net.to_inference(dtype, pyramid_dtype=...)) — keeps its
        # types: `.to(dtype)` would flatten the fp16 pyramid into the decoder's type and evaluate another configuration
        if supplied and (dtype is None or any(p_.dtype != torch.float32 for p_ in net.parameters())):
            net = net.to(device).eval()
        else:
            net = net.to(device).to(dtype).eval()
        self.net_work = net
        self.runner = None
        self.pipe = None
        if graph:
            from .runtime import ShapeCachedInference, PipelinedEvaluation
            self.runner = ShapeCachedInference(net)
            if streams > 1:
                self.pipe = PipelinedEvaluation(net, streams=streams)

    # uint8 frames [B,H,W,3] (kitti_flow.kitti_train(name, u8=True)) go to the runner, or to the network, as they came: the runner
    # keeps uint8 static inputs, and the network's first launch builds its stacked input from them — the bits of the host data
    # path's fp32 tensors cast to the network's type (ops.stack_frames_u8), inside the captured graph

    def eval_forward_stream(self, pairs):
        """pairs: iterable of (im1, im2) -> generator of flow_fw, in order, with several pairs in flight; every yielded tensor is the
        caller's own copy, as eval_forward's is.  (Not in the reference: its loop is one pair at a time.)"""
        if self.pipe is None:
            for im1, im2 in pairs:
                yield self.eval_forward(im1, im2, 0)
            return
        with torch.no_grad():
            for out in self.pipe.map(pairs):
                # (a copy, like eval_forward's: the slot's output is overwritten when the generator advances, and eval_save_result
                # — a hook whose documented purpose is to store / save predflows — may keep it; 3.7 MB per KITTI pair.  ADVICE r5)
                yield out['flow_f_out'].clone()

    def eval_forward(self, im1, im2, gt, *args):
        # === network output                                 (test.py:40-47)
        with torch.no_grad():
            if self.runner is not None:
                output_dict = self.runner(im1, im2)
                return output_dict['flow_f_out'].clone()      # (the runner owns its outputs: the caller keeps predflow across calls)
            keys = ('frames1_u8', 'frames2_u8') if torch.is_tensor(im1) and im1.dtype == torch.uint8 else ('im1', 'im2')
            output_dict = self.net_work({keys[0]: im1, keys[1]: im2, 'if_loss': False})
            return output_dict['flow_f_out']

    def eval_save_result(self, save_name, predflow, *args, **kwargs):
        if self.saver is None:
            print(save_name)
            return
        occmask = kwargs.get('occmask', args[0] if args else None)
        self.saver.submit(save_name, predflow, occmask, gt_occ_u16=kwargs.get('gt_occ_u16'), gt_noc_u16=kwargs.get('gt_noc_u16'))

    def flush(self):
        """Wait until every file handed to eval_save_result is written; re-raises the first exception of a writer thread."""
        if self.saver is not None:
            self.saver.flush()

    def close(self):
        """flush(), and end the writer threads."""
        if self.saver is not None:
            self.saver.close()


def kitti_2015_test(pretrain_path='./scripts/upflow_kitti2015.pth', dtype=torch.float32, root=None, device_score=False,
                    save_dir=None, save=('kitti',), save_workers=4, max_rad=None, png='host', error_log_colors=True, error_dilate=0):
    """device_score=True (not in the reference): undecoded items — uint8 frames, uint16 ground truth — and the metrics of every
    pair from one ops.kitti_score call on the device (Evaluation_bench(device_score=True)); the same four numbers.
    save_dir, save, save_workers, max_rad, png, error_log_colors, error_dilate: Test_model's; the files are complete when this
    returns.  save=(..., 'error') needs device_score=True (the error map is rendered from the uint16 ground truth)."""
    from .dataset.kitti_dataset import kitti_flow
    # note that eval batch size should be 1 for KITTI 2012 and KITTI 2015 (image size may be different for different sequence)
    dataset = kitti_flow.kitti_train(name='2015_train', root=root, u8=True, gt_u16=True) if device_score else None
    bench = kitti_flow.Evaluation_bench(name='2015_train', if_gpu=True, batch_size=1, root=root, dataset=dataset, device_score=device_score)
    testmodel = Test_model(pretrain_path=pretrain_path, dtype=dtype, save_dir=save_dir, save=save, save_workers=save_workers, max_rad=max_rad, png=png,
                           error_log_colors=error_log_colors, error_dilate=error_dilate)
    try:
        epe_all, f1, epe_noc, epe_occ = bench(testmodel)
    finally:
        testmodel.close()
    print('EPE All = %.2f, F1 = %.2f, EPE Noc = %.2f, EPE Occ = %.2f' % (epe_all, f1, epe_noc, epe_occ))
    return epe_all, f1, epe_noc, epe_occ


if __name__ == '__main__':
    kitti_2015_test()
