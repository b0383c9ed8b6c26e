"""Train the VAE filter on top of the frozen 2D->3D lifter (src/3d_pose_vae_filter.py).

train_step_vae is the reference's (:188-196): the lifter's evaluation forward, then loss, gradient
and Adam of the VAE alone -- here p3d_serve and one p3d_vae_train_step launch per batch.  train()
is its epoch loop (:199-296) without the plots, gen_sample_img, tqdm and the TF2 object-graph
checkpoints: the frozen lifter comes from an existing checkpoint of predict_3dpose.train
(--load N, read from --lifter_dir), the data through
predict_3dpose.load_data (the H3.6M tree and cameras or their .npz archives), and the VAE's weights
are saved as an .npz under the Keras names at the end.

    python 3d_pose_vae_filter.py --load 4874200 --lifter_dir DIR --linear_size 1024 --num_layers 2 --residual \\
        --batch_norm --camera_frame --epochs 20 --cfg_file train.yml
"""
import json
import os
import sys

import numpy as np

import predict_3dpose
from top_vae_3d_pose import losses, models
from top_vae_3d_pose.args_def import ENVIRON as ENV, filter_samples


class Adam(object):
    """tf.keras.optimizers.Adam(learning_rate): its slots and step counter live in the VAE."""

    def __init__(self, learning_rate):
        self.learning_rate = float(learning_rate)


def get_optimizer():
    """The optimizer required by flags (3d_pose_vae_filter.py:178-184)."""
    if ENV.FLAGS.optimizer == 'adam':
        return Adam(ENV.FLAGS.learning_rate)
    if ENV.FLAGS.optimizer == 'rmsprop':
        raise NotImplementedError("--optimizer rmsprop is not built (adam only)")
    raise Exception('Optimizer not found: %s' % ENV.FLAGS.optimizer)


def train_step_vae(model, x_data, y_data, optimizer, loss_out=None):
    """One training step (3d_pose_vae_filter.py:188-196): returns the device loss 3-vector."""
    f = ENV.FLAGS
    x_out = model.pose3d.serve_device(x_data)
    return model.vae.train_step_device(x_out, y_data, (f.likelihood_factor, f.kcs_factor, f.dkl_factor),
                                       optimizer.learning_rate, loss_out=loss_out)


def lifter_flags(f):
    """predict_3dpose flags of the frozen lifter from the filter's FLAGS."""
    argv = ["--linear_size", str(f.linear_size), "--num_layers", str(f.num_layers), "--batch_size", str(f.batch_size),
            "--action", f.action, "--data_dir", f.data_dir, "--cameras_path", f.cameras_path,
            "--train_dir", f.lifter_dir or f.train_dir, "--load", str(f.load), "--seed", str(f.seed)]
    for name in ("residual", "batch_norm", "max_norm", "camera_frame", "use_sh", "predict_14"):
        if getattr(f, name):
            argv.append("--" + name)
    return predict_3dpose.build_parser().parse_args(argv)


def _lifter(f):
    """The frozen lifter: checkpoint-<load> of --lifter_dir (a predict_3dpose.train run's directory),
    or fresh parameters without --load."""
    lf = lifter_flags(f)
    if f.load > 0:
        if not f.lifter_dir:
            raise ValueError("--load %d needs --lifter_dir, the directory that holds checkpoint-%d" % (f.load, f.load))
        ck = os.path.join(f.lifter_dir, "checkpoint-%d" % f.load)
        if not (os.path.isfile(ck + ".index") or os.path.isfile(ck + ".npz")):
            raise ValueError("Asked to load checkpoint {0}, but it does not seem to exist".format(f.load))
        lf.load = 0
        model = predict_3dpose.create_model(None, None, lf.batch_size, lf)
        print("Loading lifter {0}".format(ck))
        model.saver.restore(None, ck)
        return model, lf
    print("No --load: the lifter keeps fresh parameters (the reference loads its pretrained PoseBase)")
    return predict_3dpose.create_model(None, None, lf.batch_size, lf), lf


def _epoch_batches(model, d, lf, training):
    import torch
    enc, dec = model.pose3d.get_all_batches(d["train_set_2d" if training else "test_set_2d"],
                                            d["train_set_3d" if training else "test_set_3d"], lf.camera_frame,
                                            training=training)
    if not enc:
        return None, None, 0
    dev = model.pose3d.device
    X = torch.from_numpy(np.ascontiguousarray(np.concatenate(enc), dtype=np.float32)).to(dev)
    Y = torch.from_numpy(np.ascontiguousarray(np.concatenate(dec), dtype=np.float32)).to(dev)
    return X, Y, len(enc)


def train(argv=None, read_from_config=False):
    """Epoch loop of 3d_pose_vae_filter.py:199-296.  Returns (model, history) with history the
    per-epoch lists loss_train, loss_test (3-vectors), error_3d_out and error_vae_out."""
    import torch
    f = ENV.setup(read_from_config=read_from_config, argv=argv)
    if f.train_all:
        raise NotImplementedError("--train_all is not built: the lifter stays frozen")
    if f.sample:
        raise NotImplementedError("--sample (gen_sample_img) is matplotlib visualisation, not built")
    K = filter_samples(f)      # the test block's VAE output: None, one draw; else the mean of K samples
    pose3d, lf = _lifter(f)
    d = predict_3dpose.load_data(lf)
    model = models.Pose3DVae(latent_dim=f.latent_dim, enc_dim=f.enc_dim, dec_dim=f.dec_dim, pose3d=pose3d,
                             max_batch=max(f.batch_size, 4096), seed=f.seed)
    optimizer = get_optimizer()
    print("Training only VAE weights:", len(model.vae.param_table))
    print("Plots, sample images, progress bars and TF2 checkpoints are left out of this build")
    B = f.batch_size
    hist = {"loss_train": [], "loss_test": [], "error_3d_out": [], "error_vae_out": []}
    for epoch in range(1, f.epochs + 1):
        print("\nStarting epoch:", epoch)
        X, Y, nb = _epoch_batches(model, d, lf, training=True)
        step_losses = torch.zeros((max(nb, 1), 3), dtype=torch.float32, device=pose3d.device)
        for step in range(nb):
            train_step_vae(model, X[step * B:(step + 1) * B], Y[step * B:(step + 1) * B], optimizer,
                           loss_out=step_losses[step])
            if step % f.step_log == 0:
                print(" Training loss at step %d: %.4f" % (step, float(step_losses[step].mean().item())))
                print(" Seen : %s samples" % ((step + 1) * B))
        hist["loss_train"].append(step_losses[:nb].double().mean(dim=0).cpu().numpy())
        print("Evaluation on Test data...")
        X, Y, nb = _epoch_batches(model, d, lf, training=False)
        lt = torch.zeros((max(nb, 1), 3), dtype=torch.float32, device=pose3d.device)
        e3, ev = [], []
        for step in range(nb):
            xb, yb = X[step * B:(step + 1) * B], Y[step * B:(step + 1) * B]
            out_3d, out_vae = model(xb, training=False) if K is None else model(xb, training=False, samples=K)
            lt[step].copy_(losses.ELBO.compute_loss(model.vae, out_3d, yb))
            a, b = losses.ELBO.compute_error_3d_vs_vae(yb, out_3d, out_vae)
            e3.append(a)
            ev.append(b)
        hist["loss_test"].append(lt[:nb].double().mean(dim=0).cpu().numpy())
        hist["error_3d_out"].append(float(torch.stack(e3).mean().item()) if e3 else float("nan"))
        hist["error_vae_out"].append(float(torch.stack(ev).mean().item()) if ev else float("nan"))
        print('Epoch: {}, Test set ELBO: {}'.format(epoch, hist["loss_test"][-1]))
        print('Error real vs 3d out:', hist["error_3d_out"][-1])
        print('Error real vs vae out:', hist["error_vae_out"][-1])
    out_dir = os.path.join(ENV.TRAIN_DIR, "3d_vae")
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
