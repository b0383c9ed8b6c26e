"""Train the stand-alone VAE denoiser (src/vae_filter.py): a 48 -> 48 VAE that reads a 3D pose
under data_handler's noise and returns the clean one.

train() is the reference's epoch loop (:136-218) without the plots and the TF2 checkpoints; with
--samples_dir DIR it writes, where the reference calls gen_sample_img (:198-200), the numbers behind
that picture to DIR/samples_<epoch>.npz (top_vae_3d_pose/samples.py).  All 3D poses are joined,
shuffled and split 80/20 (data_handler.load_3d_data) and live on the device; both halves are noised there (data_handler.Dataset, p3d_vae_add_noise) and re-noised
after every epoch, so an epoch moves no data between host and device: a batch is two device gathers
and one p3d_vae_train_step launch.

The reference's script is stale against its own package: it reads ``FLAGS.vae_dim`` and passes
``inter_dim=`` to a VAE that takes ``enc_dim`` / ``dec_dim``.  Here the shape comes from
--enc_dim / --latent_dim / --dec_dim, as in the other drivers.  --noised_sample and --sample are
matplotlib visualisation and raise NotImplementedError (--samples_dir gives their numbers).

    python vae_filter.py --camera_frame --epochs 20 --cfg_file train.yml
"""
import importlib.util
import json
import os
import sys

import predict_3dpose
from top_vae_3d_pose import data_handler, losses, models, samples
from top_vae_3d_pose.args_def import ENVIRON as ENV, filter_samples


def _base():
    """3d_pose_vae_filter.py (its name is no Python identifier): lifter_flags, get_optimizer."""
    if "pose_vae_filter" not in sys.modules:
        spec = importlib.util.spec_from_file_location(
            "pose_vae_filter", os.path.join(os.path.dirname(os.path.abspath(__file__)), "3d_pose_vae_filter.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["pose_vae_filter"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["pose_vae_filter"]


def weights_path():
    return os.path.join(ENV.TRAIN_DIR, "vae", "last_model_weights")


def train(argv=None, read_from_config=False):
    """Epoch loop of vae_filter.py:136-218.  Returns (model, history) with history the per-epoch
    lists loss_train, loss_test (3-vectors), error_pred and error_noised; the two Datasets are
    model.data_train and model.data_test."""
    import torch
    f = ENV.setup(read_from_config=read_from_config, argv=argv)
    K = filter_samples(f)      # the test block's VAE output: None, one draw; else the mean of K samples
    if f.noised_sample:
        raise NotImplementedError("--noised_sample (gen_sample_img) is matplotlib visualisation, not built; "
                                  "--samples_dir DIR writes the sample sets it would draw")
    if f.sample:
        raise NotImplementedError("--sample (gen_sample_img) is matplotlib visualisation, not built; "
                                  "--samples_dir DIR writes the sample sets it would draw")
    base = _base()
    optimizer = base.get_optimizer()
    d = predict_3dpose.load_data(base.lifter_flags(f))
    data_train, data_test = data_handler.load_3d_data(d)
    print("Dataset dims")
    print(data_train.shape, data_test.shape)
    B = f.batch_size
    model = models.VAE(data_train.shape[1], latent_dim=f.latent_dim, enc_dim=f.enc_dim, dec_dim=f.dec_dim,
                       human_3d_size=data_train.shape[1], max_batch=max(B, 4096), seed=f.seed)
    model.data_train, model.data_test = data_train, data_test
    print("Trainable weights:", len(model.param_table))
    print("Plots, sample images, progress bars and TF2 checkpoints are left out of this build")
    dev = model.device
    factors = (f.likelihood_factor, f.kcs_factor, f.dkl_factor)
    hist = {k: [] for k in ("loss_train", "loss_test", "error_pred", "error_noised")}
    idx = None
    if f.samples_dir:   # Indexes for sampling (:157): one draw, before the first epoch
        import numpy as np
        os.makedirs(f.samples_dir, exist_ok=True)
        idx = np.random.choice(data_test.shape[0], samples.NSAMPLES, replace=False)
    for epoch in range(1, f.epochs + 1):
        print("\nStarting epoch:", epoch)
        nb = len(data_train)
        step_losses = torch.zeros((max(nb, 1), 3), dtype=torch.float32, device=dev)
        for step, (x_noised, x_truth) in enumerate(data_train):
            model.train_step_device(x_noised, x_truth, factors, optimizer.learning_rate, loss_out=step_losses[step])
            if step % f.step_log == 0:
                print(" Training loss at step %d: %.4f" % (step, float(step_losses[step].mean().item())))
                print(" Seen : %s samples" % ((step + 1) * B))
        hist["loss_train"].append(step_losses[:nb].double().mean(dim=0).cpu().numpy())
        nb = len(data_test)
        lt = torch.zeros((max(nb, 1), 3), dtype=torch.float32, device=dev)
        err_n, err_p = [], []
        for step, (x_noised, x_truth) in enumerate(data_test):
            lt[step].copy_(losses.ELBO.compute_loss(model, x_noised, x_truth))
            err_n.append(losses.ELBO.compute_pred_error(x_noised, x_truth))
            pred = model(x_noised, training=False) if K is None else model(x_noised, training=False, samples=K)
            err_p.append(losses.ELBO.compute_pred_error(pred, x_truth))
        hist["loss_test"].append(lt[:nb].double().mean(dim=0).cpu().numpy())
        hist["error_noised"].append(float(torch.stack(err_n).mean().item()) if err_n else float("nan"))
        hist["error_pred"].append(float(torch.stack(err_p).mean().item()) if err_p else float("nan"))
        print('Epoch: {}, Test set ELBO: {}'.format(epoch, hist["loss_test"][-1]))
        print('Error real vs noised:', hist["error_noised"][-1])
        print('Error real vs pred:', hist["error_pred"][-1])
        if idx is not None:
            print('\nSaving samples...')
            meta = data_test.metadata
            samples.gen_samples(model, data_test.data, data_test.data_noised, meta.mean, meta.std, meta.dim_ignored,
                                idx=idx, path=samples.sample_path(f.samples_dir, epoch))
        # Reset data for next epoch
        data_train.on_epoch_end(new_noise=True)
        data_test.on_epoch_end(new_noise=True)
    os.makedirs(os.path.dirname(weights_path()), exist_ok=True)
    model.save_weights(weights_path())
    with open(os.path.join(os.path.dirname(weights_path()), "train.cfg"), "w") as cfg:
        json.dump(vars(f), cfg)
    print("Weights saved:", weights_path() + ".npz")
    return model, hist


def main():
    model, _ = train(sys.argv[1:], read_from_config="--cfg_file" in " ".join(sys.argv[1:]))
    model.close()


if __name__ == "__main__":
    main()
