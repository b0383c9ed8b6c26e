"""Train the VAE filter over [x2d, out_3d, effnet_out] on top of the frozen 2D->3D lifter
(src/3d_pose_effnet_2d_vae_filter.py): the 1360-input filter of models.py:485-540 built with
use_2d=True, use_effnet_ouptut=True.

train() is the reference's epoch loop (:171-301) in the style of 3d_pose_vae_filter.py: the frozen
lifter comes from --load / --lifter_dir, X / Y are built in key order, the precomputed EfficientNet
features (--effnet_outputs_path, data_handler.load_effnet_outputs) are loaded ONCE onto the device
in the same order, and an epoch draws a device permutation: X / Y are gathered once per epoch, the
feature table is never copied -- every batch indexes it in place, inside the filter's kernels, by
its slice of the permutation.  A step is p3d_serve and one train_step_device([x, out_3d, (F, idx)]).
Plots, gen_sample_img, tqdm and the TF2 checkpoints are left out; the weights are saved as an .npz
under the Keras names in 3d_effnet_2d_vae/.

The reference joins train and test, reshuffles and re-splits them (load_2d_3d_data); this build
keeps the project's split by subject (predict_3dpose.load_data).

    python 3d_pose_effnet_2d_vae_filter.py --load 4874200 --lifter_dir DIR --linear_size 1024 --num_layers 2 \\
        --residual --batch_norm --camera_frame --epochs 20 --cfg_file train.yml --effnet_outputs_path effnet.npz
"""
import importlib.util
import json
import os
import sys

import numpy as np

import predict_3dpose
from top_vae_3d_pose import data_handler, losses, models
from top_vae_3d_pose.args_def import ENVIRON as ENV, filter_samples

_spec = importlib.util.spec_from_file_location(
    "pose_vae_filter", os.path.join(os.path.dirname(os.path.abspath(__file__)), "3d_pose_vae_filter.py"))
base = importlib.util.module_from_spec(_spec)     # the sibling driver: get_optimizer, the frozen lifter
_spec.loader.exec_module(base)


def train_step_vae(model, x_data, y_data, effnet, optimizer, loss_out=None):
    """One training step (3d_pose_effnet_2d_vae_filter.py:158-168): the device loss 3-vector.
    `effnet` is a [B, effnet_size] tensor or (table, idx)."""
    f = ENV.FLAGS
    out_3d = model.pose3d.serve_device(x_data)
    return model.vae.train_step_device(model.segments(x_data, out_3d, effnet), y_data,
                                       (f.likelihood_factor, f.kcs_factor, f.dkl_factor),
                                       optimizer.learning_rate, loss_out=loss_out)


def key_order_arrays(data_x, data_y, camera_frame):
    """X [n, 32], Y [n, 48] with the dict's keys concatenated in order (linear_model.get_all_batches
    without its permutation and tail cut), and the keys and their 2D frame counts."""
    keys, sizes, xs, ys = [], [], [], []
    for key2d in data_x.keys():
        subj, b, fname = key2d
        key3d = key2d if camera_frame else (subj, b, '{0}.h5'.format(fname.split('.')[0]))
        key3d = (subj, b, fname[:-3]) if fname.endswith('-sh') and camera_frame else key3d
        keys.append((subj, b, fname[:-3] if fname.endswith('-sh') else fname))
        sizes.append(data_x[key2d].shape[0])
        xs.append(data_x[key2d])
        ys.append(data_y[key3d])
    return (np.ascontiguousarray(np.concatenate(xs), dtype=np.float32),
            np.ascontiguousarray(np.concatenate(ys), dtype=np.float32), keys, sizes)


def _device_split(d, lf, which, path, dev):
    import torch
    X, Y, keys, sizes = key_order_arrays(d[which + "_set_2d"], d[which + "_set_3d"], lf.camera_frame)
    F = data_handler.load_effnet_outputs(path, keys, sizes)
    assert F.shape[0] == X.shape[0]
    return (torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev),
            torch.from_numpy(np.ascontiguousarray(F, dtype=np.float32)).to(dev))


def train(argv=None, read_from_config=False):
    """Epoch loop of 3d_pose_effnet_2d_vae_filter.py:171-301.  Returns (model, history) with history
    the per-epoch lists loss_train, loss_test (3-vectors), error_3d_out and error_vae_out."""
    import torch
    f = ENV.setup(read_from_config=read_from_config, argv=argv)
    if f.train_all:
        raise NotImplementedError("--train_all is not built: the lifter stays frozen")
    if f.sample:
        raise NotImplementedError("--sample (gen_sample_img) is matplotlib visualisation, not built")
    K = filter_samples(f)      # the test block's VAE output: None, one draw; else the mean of K samples
    if f.use_effb1:
        print("--use_effb1 is accepted and ignored: the features are read precomputed from", f.effnet_outputs_path)
    optimizer = base.get_optimizer()
    pose3d, lf = base._lifter(f)
    d = predict_3dpose.load_data(lf)
    dev = pose3d.device
    X, Y, F = _device_split(d, lf, "train", f.effnet_outputs_path, dev)
    Xt, Yt, Ft = _device_split(d, lf, "test", f.effnet_outputs_path, dev)
    model = models.Pose3DVaeCat(latent_dim=f.latent_dim, enc_dim=f.enc_dim, dec_dim=f.dec_dim, use_effnet_ouptut=True,
                                use_2d=True, pose3d=pose3d, effnet_size=int(F.shape[1]),
                                max_batch=max(f.batch_size, 4096), seed=f.seed)
    print("Training only VAE weights:", len(model.vae.param_table))
    print("Plots, sample images, progress bars and TF2 checkpoints are left out of this build")
    B = f.batch_size
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(f.seed))
    hist = {"loss_train": [], "loss_test": [], "error_3d_out": [], "error_vae_out": []}
    for epoch in range(1, f.epochs + 1):
        print("\nStarting epoch:", epoch)
        n = X.shape[0]
        nb = n // B
        perm = torch.randperm(n, device=dev, generator=gen)
        Xp, Yp = X[perm], Y[perm]          # one gather per epoch; the feature table stays where it is
        step_losses = torch.zeros((max(nb, 1), 3), dtype=torch.float32, device=dev)
        for step in range(nb):
            sl = slice(step * B, (step + 1) * B)
            train_step_vae(model, Xp[sl], Yp[sl], (F, perm[sl]), optimizer, loss_out=step_losses[step])
            if step % f.step_log == 0:
                print(" Training loss at step %d: %.4f" % (step, float(step_losses[step].mean().item())))
                print(" Seen : %s samples" % ((step + 1) * B))
        hist["loss_train"].append(step_losses[:nb].double().mean(dim=0).cpu().numpy())
        print("Evaluation on Test data...")
        nbt = Xt.shape[0] // B
        lt = torch.zeros((max(nbt, 1), 3), dtype=torch.float32, device=dev)
        e3, ev = [], []
        for step in range(nbt):
            sl = slice(step * B, (step + 1) * B)
            xb, yb, fb = Xt[sl], Yt[sl], Ft[sl]
            out_3d, out_vae = (model(xb, effnet_output=fb, training=False) if K is None else
                               model(xb, effnet_output=fb, training=False, samples=K))
            lt[step].copy_(losses.ELBO.compute_loss(model.vae, model.segments(xb, out_3d, fb), yb))
            a, b = losses.ELBO.compute_error_3d_vs_vae(yb, out_3d, out_vae)
            e3.append(a)
            ev.append(b)
        hist["loss_test"].append(lt[:nbt].double().mean(dim=0).cpu().numpy())
        hist["error_3d_out"].append(float(torch.stack(e3).mean().item()) if e3 else float("nan"))
        hist["error_vae_out"].append(float(torch.stack(ev).mean().item()) if ev else float("nan"))
        print('Epoch: {}, Test set ELBO: {}'.format(epoch, hist["loss_test"][-1]))
        print('Error real vs 3d out:', hist["error_3d_out"][-1])
        print('Error real vs vae out:', hist["error_vae_out"][-1])
    out_dir = os.path.join(ENV.TRAIN_DIR, "3d_effnet_2d_vae")
    os.makedirs(out_dir, exist_ok=True)
    model.save_weights(os.path.join(out_dir, "last_model_weights"))
    with open(os.path.join(out_dir, "train.cfg"), "w") as cfg:
        json.dump(vars(f), cfg)
    print("Weights saved:", os.path.join(out_dir, "last_model_weights.npz"))
    return model, hist


def main():
    model, _ = train(sys.argv[1:], read_from_config="--cfg_file" in " ".join(sys.argv[1:]))
    model.close()
    model.pose3d.close()


if __name__ == "__main__":
    main()
