"""nnUNet_train for nnUNetTrainerV2_noDataAugmentation on the stock 2-D Generic_UNet, on the device.

    python -m cineflow.train --plans PLANS_PKL --data STAGE_FOLDER -o EXPERIMENT -f FOLD
        [--splits FILE] [--epochs N] [--batches_per_epoch N] [--val_batches N] [--seed S] [-c]

Restated from nnunet/training/network_training: nnUNet_variants/data_augmentation/nnUNetTrainerV2_noDA.py on nnUNetTrainerV2.py:47-53,
62-175, 231-279, 364, 421-430, nnUNetTrainer.py:278 and network_trainer.py:108-109, 516-540 -- initial_lr 1e-2, weight decay 3e-5, 1000
epochs of 250 training and 50 validation batches, poly_lr(ep, max, lr0, 0.9) at each epoch's start, SGD(momentum 0.99, nesterov),
clip_grad_norm_(12) before each step, the fp32 branch of run_iteration, deep-supervision weights 1 / 2**i with the lowest resolution zeroed.
The loader restates DataLoader2D.generate_train_batch (dataloading/dataset_loading.py:470-700) under get_no_augmentation: cases drawn with
replacement, the last batch - round(batch * (1 - 0.33)) elements forced to foreground, a random crop of the plans' patch size, data padded
with 0 and seg with -1, RemoveLabelTransform(-1, 0).

The result is a segmentation-only model folder (plans.json, fold_X/model_final_checkpoint.model) that cineflow.validate and cineflow.predict
load unchanged; its plans record mirror_axes = () as the noDA trainer does.  What is not built: DESIGN.md section 8."""
import argparse
import collections
import concurrent.futures
import json
import os
import time

import numpy as np
import torch

from . import ops, train_ops as T
from .train_net import TrainNet, check_servable, deep_supervision_scales, deep_supervision_weights

join = os.path.join
MAX_LOADER_THREADS = 16


def poly_lr(epoch, max_epochs, initial_lr, exponent=0.9):
    return initial_lr * (1 - epoch / max_epochs) ** exponent


# ------------------------------------------------------------------------------------------------ loader
class Loader2D(object):
    """DataLoader2D + get_no_augmentation on the host.  Every random decision of a batch is drawn from `rng` in the calling thread, in
    batch order, before any worker touches the batch ("plan"); the workers only crop and pad ("fill").  So the batches do not depend on the
    thread count, and the generator state that belongs to the next unconsumed batch is known at any time (state())."""

    def __init__(self, dataset, keys, patch_size, batch_size, rng, oversample_foreground_percent=0.33, threads=8, prefetch=2):
        self.dataset, self.keys = dataset, list(keys)
        self.patch = tuple(int(v) for v in patch_size)
        self.batch_size, self.rng, self.oversample = int(batch_size), rng, oversample_foreground_percent
        self.threads = max(1, min(int(threads), MAX_LOADER_THREADS))
        self.prefetch = max(0, int(prefetch))
        self.pool = concurrent.futures.ThreadPoolExecutor(self.threads)
        self.pending = collections.deque()               # (generator state before the plan, plan, [futures])
        self._cases = {}

    def case(self, key):
        """(data [C+1, D, H, W] with the segmentation last, properties); kept in memory once read"""
        if key not in self._cases:
            from .safe_pickle import load_plain_pickle
            entry = self.dataset[key]
            npy = entry["data_file"][:-4] + ".npy"
            data = np.load(npy, "r") if os.path.isfile(npy) else np.load(entry["data_file"])["data"]
            if data.ndim == 3:
                data = data[:, None]
            self._cases[key] = (data, entry["properties"] if "properties" in entry else load_plain_pickle(entry["properties_file"]))
        return self._cases[key]

    def get_do_oversample(self, j):
        return not j < round(self.batch_size * (1 - self.oversample))

    def plan_batch(self):
        """-> [(case, slice, (y0, x0), forced to foreground)] of the next batch; consumes the generator"""
        rng = self.rng
        picks = rng.integers(0, len(self.keys), size=self.batch_size)
        plan = []
        for j, i in enumerate(picks):
            key = self.keys[int(i)]
            data, props = self.case(key)
            force_fg, voxels = self.get_do_oversample(j), None
            if force_fg:
                if "class_locations" not in props:
                    raise RuntimeError("%s has no class_locations: rerun the preprocessing" % key)
                loc = props["class_locations"]
                fg = sorted(int(c) for c in loc.keys() if len(loc[c]) != 0 and int(c) > 0)
                if fg:
                    cls = fg[int(rng.integers(len(fg)))]
                    vox = np.asarray({int(k): v for k, v in loc.items()}[cls])
                    valid = np.unique(vox[:, 0])
                    sl = int(valid[int(rng.integers(len(valid)))])
                    voxels = vox[vox[:, 0] == sl][:, 1:]
            if voxels is None:
                sl = int(rng.integers(data.shape[1]))
            shape = data.shape[2:]
            lb, ub = [], []
            for d in range(2):
                need = max(self.patch[d] - shape[d], 0)
                lb.append(-(need // 2))
                ub.append(shape[d] + need // 2 + need % 2 - self.patch[d])
            if voxels is None:
                box = tuple(int(rng.integers(lb[d], ub[d] + 1)) for d in range(2))
            else:
                v = voxels[int(rng.integers(len(voxels)))]
                box = tuple(max(lb[d], int(v[d]) - self.patch[d] // 2) for d in range(2))
            plan.append((key, sl, box, bool(force_fg)))
        return plan

    def fill(self, item):
        key, sl, (y0, x0), _forced = item
        data, _props = self.case(key)
        img = data[:, sl]
        H, W = img.shape[1:]
        ph, pw = self.patch
        vy0, vy1, vx0, vx1 = max(0, y0), min(H, y0 + ph), max(0, x0), min(W, x0 + pw)
        out = np.zeros((img.shape[0] - 1, ph, pw), np.float32)
        seg = np.full((ph, pw), -1, np.float32)
        out[:, vy0 - y0:vy1 - y0, vx0 - x0:vx1 - x0] = img[:-1, vy0:vy1, vx0:vx1]
        seg[vy0 - y0:vy1 - y0, vx0 - x0:vx1 - x0] = img[-1, vy0:vy1, vx0:vx1]
        seg[seg == -1] = 0                                # RemoveLabelTransform(-1, 0)
        return out, seg.astype(np.int32)

    def _submit(self):
        state = self.rng.bit_generator.state
        plan = self.plan_batch()
        self.pending.append((state, plan, [self.pool.submit(self.fill, it) for it in plan]))

    def __next__(self):
        while len(self.pending) < self.prefetch + 1:
            self._submit()
        _state, plan, futures = self.pending.popleft()
        parts = [f.result() for f in futures]
        return {"data": np.stack([p[0] for p in parts]), "seg": np.stack([p[1] for p in parts]), "plan": plan}

    next = __next__

    def state(self):
        """the generator state from which the next unconsumed batch is drawn"""
        return self.pending[0][0] if self.pending else self.rng.bit_generator.state

    def set_state(self, state):
        for _s, _p, futures in self.pending:
            for f in futures:
                f.result()
        self.pending.clear()
        self.rng.bit_generator.state = state

    def close(self):
        self.pool.shutdown(wait=True)


def make_generators(seed):
    """one seed -> the training and the validation loader's generator (two streams of one SeedSequence)"""
    return [np.random.Generator(np.random.PCG64(s)) for s in np.random.SeedSequence(int(seed)).spawn(2)]


# ------------------------------------------------------------------------------------------------ trainer
class SegTrainer(object):
    initial_lr = 1e-2
    weight_decay = 3e-5
    momentum = 0.99
    clip_norm = 12.0
    save_latest_every = 50

    def __init__(self, plans_file, data_folder, output_folder, fold, splits_file=None, max_num_epochs=1000, num_batches_per_epoch=250,
                 num_val_batches_per_epoch=50, seed=12345, threads=8, device=None, batch_dice=True):
        if not batch_dice:
            raise ValueError("batch_dice=False is refused: the reference's loss is then a vector of length B and its backward() cannot run")
        self.plans_file, self.data_folder, self.output_folder, self.fold = plans_file, data_folder, output_folder, fold
        self.splits_file = splits_file or join(os.path.dirname(os.path.abspath(data_folder.rstrip("/"))), "splits_final.pkl")
        self.max_num_epochs, self.num_batches_per_epoch = int(max_num_epochs), int(num_batches_per_epoch)
        self.num_val_batches_per_epoch, self.seed, self.threads = int(num_val_batches_per_epoch), int(seed), int(threads)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.fold_name = "fold_%s" % fold if str(fold) == "all" else "fold_%d" % int(fold)
        self.epoch, self.first_step = 0, True
        self.was_initialized = False

    # -- nnUNetTrainerV2.initialize
    def initialize(self, training=True):
        from .reference_models import load_reference_pickle, plans_from_reference
        from .validate import do_split, load_dataset
        ref_plans = load_reference_pickle(self.plans_file)
        self.plans = plans_from_reference(ref_plans)
        self.plans["mirror_axes"] = []                   # nnUNetTrainerV2_noDA: do_mirroring False at validation
        check_servable(self.plans)
        stage = list(ref_plans["plans_per_stage"].values())[0]      # plans_from_reference(stage=None) admits exactly one
        self.batch_size = int(stage["batch_size"])
        self.patch_size = self.plans["patch_size"]
        sk = self.plans["seg_net"]
        self.num_classes = self.plans["num_classes"]
        self.net = TrainNet(self.plans["num_modalities"], sk["base_num_features"], self.num_classes, sk["num_pool"],
                            pool_op_kernel_sizes=sk["pool_op_kernel_sizes"]).to(self.device)
        self.net.init_weights(self.seed)
        self.ds_weights = [float(w) for w in deep_supervision_weights(sk["num_pool"])]
        self.ds_scales = deep_supervision_scales(sk["pool_op_kernel_sizes"])
        self.no_grad = None
        if training:
            self.dataset = load_dataset(self.data_folder)
            tr_keys, val_keys = do_split(self.dataset.keys(), self.fold, self.splits_file)
            rng_tr, rng_val = make_generators(self.seed)
            self.tr_gen = Loader2D(self.dataset, tr_keys, self.patch_size, self.batch_size, rng_tr, threads=self.threads)
            self.val_gen = Loader2D(self.dataset, val_keys, self.patch_size, self.batch_size, rng_val, threads=max(1, self.threads // 2))
            os.makedirs(join(self.output_folder, self.fold_name), exist_ok=True)
        self.was_initialized = True

    def targets(self, seg):
        """DownsampleSegForDSTransform2 at order 0: one int32 label map per output, full resolution first"""
        from .preprocessing import resize_segmentation
        seg = seg.to(self.device)
        out = []
        for s in self.ds_scales:
            if all(v == 1 for v in s):
                out.append(seg.contiguous())
                continue
            shp = [int(v) for v in np.round(np.array(seg.shape[1:]) * np.array(s))]
            out.append(torch.stack([resize_segmentation(seg[b], shp, order=0) for b in range(seg.shape[0])]).contiguous())
        return out

    def maybe_update_lr(self, epoch=None):
        ep = self.epoch if epoch is None else epoch
        self.lr = poly_lr(ep, self.max_num_epochs, self.initial_lr, 0.9)
        return self.lr

    # -- nnUNetTrainerV2.run_iteration, fp32 branch
    def run_iteration(self, data_generator, do_backprop=True, run_online_evaluation=False):
        """-> the loss as a device scalar (no host read: callers read it when they log)"""
        batch = next(data_generator)
        data = torch.from_numpy(batch["data"]).to(self.device)
        targets = self.targets(torch.from_numpy(batch["seg"]))
        outputs = self.net.forward_train(data)
        loss, dl = T.deep_supervision_loss(outputs, targets, self.ds_weights, want_grad=do_backprop)
        if do_backprop:
            no_grad = self.net.backward(dl)
            table = self.net.table(no_grad)
            clip = T.grad_norm(self.net.grad, table, len(self.net.names), self.clip_norm)
            T.sgd_nesterov(self.net.param, self.net.grad, self.net.mom, table, len(self.net.names), self.net.max_tensor, clip, self.lr,
                           self.weight_decay, self.momentum, first=self.first_step)
            self.first_step = False
        else:
            self.net.records = None
        if run_online_evaluation:
            self.run_online_evaluation(outputs[0], targets[0])
        return loss

    def run_online_evaluation(self, output, target):
        """nnUNetTrainer.run_online_evaluation: hard arg-max of the full-resolution output, foreground tp / fp / fn summed over the epoch"""
        from .metrics import label_confusion
        m = label_confusion(ops.argmax_channels(output), target.to(torch.uint8), self.num_classes)      # m[test, reference]
        tp = np.diag(m)[1:]
        self.online_tp += tp
        self.online_fp += m.sum(1)[1:] - tp
        self.online_fn += m.sum(0)[1:] - tp

    def finish_online_evaluation(self):
        """global Dice per foreground class over the epoch's validation batches (classes that never occur are left out of the mean)"""
        tp, fp, fn = self.online_tp, self.online_fp, self.online_fn
        dc = [2 * i / (2 * i + j + k) for i, j, k in zip(tp, fp, fn) if 2 * i + j + k > 0]
        return float(np.mean(dc)) if dc else float("nan")

    def on_epoch_end(self, train_loss, val_loss, dice):
        line = "epoch %d lr %.6g train_loss %.6f val_loss %.6f mean_fg_dice %.6f" % (self.epoch, self.lr, train_loss, val_loss, dice)
        with open(join(self.output_folder, self.fold_name, "training_log.txt"), "a") as f:
            f.write(line + "\n")
        print(line)
        self.epoch += 1
        if self.epoch % self.save_latest_every == 0 and self.epoch < self.max_num_epochs:
            self.save_checkpoint("model_latest")
        return self.epoch < self.max_num_epochs

    def run_training(self):
        if not self.was_initialized:
            self.initialize(True)
        while self.epoch < self.max_num_epochs:
            self.maybe_update_lr()
            tl = [self.run_iteration(self.tr_gen, True) for _ in range(self.num_batches_per_epoch)]
            self.online_tp, self.online_fp, self.online_fn = (np.zeros(self.num_classes - 1, np.int64) for _ in range(3))
            vl = [self.run_iteration(self.val_gen, False, True) for _ in range(self.num_val_batches_per_epoch)]
            mean = lambda ls: float(torch.stack(ls).mean()) if ls else float("nan")      # noqa: E731  (the epoch's one host read of losses)
            self.on_epoch_end(mean(tl), mean(vl), self.finish_online_evaluation())
        self.save_checkpoint("model_final_checkpoint")
        self.tr_gen.close()
        self.val_gen.close()

    # -- checkpoints: weights in the reference's state_dict layout (a model folder validate / predict load), training state beside them
    def save_checkpoint(self, name="model_latest"):
        from .trainer import save_model_folder
        fold = "all" if str(self.fold) == "all" else int(self.fold)
        if fold == "all":                                   # save_model_folder formats fold_%d
            os.makedirs(join(self.output_folder, "fold_all"), exist_ok=True)
            with open(join(self.output_folder, "plans.json"), "w") as f:
                json.dump(self.plans, f, indent=1)
            torch.save({"seg_state_dict": self.net.state_dict()}, join(self.output_folder, "fold_all", name + ".model"))
        else:
            save_model_folder(self.output_folder, None, None, self.plans, fold=fold, checkpoint_name=name, seg_sd=self.net.state_dict())
        state = {"momentum": self.net.mom.cpu(), "epoch": self.epoch, "first_step": self.first_step,
                 "rng": json.dumps([self.tr_gen.state(), self.val_gen.state()])}
        torch.save(state, join(self.output_folder, self.fold_name, name + ".train"))

    def load_checkpoint(self, name=None):
        folder = join(self.output_folder, self.fold_name)
        if name is None:
            name = next((n for n in ("model_final_checkpoint", "model_latest") if os.path.isfile(join(folder, n + ".train"))), None)
            if name is None:
                raise FileNotFoundError("no checkpoint to continue from in %s" % folder)
        ck = torch.load(join(folder, name + ".model"), map_location="cpu", weights_only=True)
        st = torch.load(join(folder, name + ".train"), map_location="cpu", weights_only=True)
        self.net.load_state_dict(ck["seg_state_dict"])
        self.net.mom.copy_(st["momentum"])
        self.epoch, self.first_step = int(st["epoch"]), bool(st["first_step"])
        tr, val = json.loads(st["rng"])
        self.tr_gen.set_state(tr)
        self.val_gen.set_state(val)


def build_parser():
    p = argparse.ArgumentParser(description="train one fold of nnUNetTrainerV2_noDataAugmentation (2-D Generic_UNet) on the device")
    p.add_argument("--plans", required=True, help="the task's nnUNetPlansv2.1_plans_2D.pkl")
    p.add_argument("--data", required=True, help="stage folder of the preprocessed task (<case>.npz / <case>.pkl)")
    p.add_argument("-o", "--output_folder", required=True, help="EXPERIMENT: the model folder to write")
    p.add_argument("-f", "--fold", required=True, help="fold number, or all")
    p.add_argument("--splits", default=None, help="splits_final.pkl (default: next to the stage folder; created when absent)")
    p.add_argument("--epochs", type=int, default=1000)
    p.add_argument("--batches_per_epoch", type=int, default=250)
    p.add_argument("--val_batches", type=int, default=50)
    p.add_argument("--seed", type=int, default=12345)
    p.add_argument("--threads", type=int, default=8, help="loader threads (at most %d); the batches do not depend on it" % MAX_LOADER_THREADS)
    p.add_argument("-c", "--continue_training", action="store_true", help="continue from the fold's latest checkpoint")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.fold != "all":
        int(a.fold)
    t = SegTrainer(a.plans, a.data, a.output_folder, a.fold, a.splits, a.epochs, a.batches_per_epoch, a.val_batches, a.seed, a.threads)
    t.initialize(True)
    if a.continue_training:
        t.load_checkpoint()
    t0 = time.time()
    t.run_training()
    print("done: %d epochs in %.1f s -> %s" % (t.epoch, time.time() - t0, join(a.output_folder, t.fold_name, "model_final_checkpoint.model")))


if __name__ == "__main__":
    main()
