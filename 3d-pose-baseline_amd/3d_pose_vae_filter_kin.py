"""Train and evaluate the temporal VAE filter (src/3d_pose_vae_filter_kin.py): a VAE that reads the
last three 3D poses concatenated (144 inputs) and returns the refined last one.

train() (:158-280) trains it as a denoiser on sliding windows of the 3D sequences
(data_handler.load_dataset_3d_seq) under data_handler.add_noise -- one p3d_vae_train_step launch per
batch -- without the plots, gen_sample_img, tqdm and the TF2 checkpoints.  Per epoch the shuffled
windows are gathered on the device with a torch index and noised ONCE over the whole epoch on the
host; the reference draws its noise batch by batch, so the np.random stream differs and the noise's
distribution does not.  With --device_noise the epoch's windows are instead read in place and noised
on the GPU by one data_handler.add_noise_device call (p3d_vae_add_noise, keyed by --seed and the
epoch): nothing is copied to the host and np.random draws only the epoch's permutation.

evaluate() (:285-361) runs the filter the way it is used: as a recurrence over every test sequence
on top of the frozen lifter, each frame's refined pose written back into the buffer that feeds the
next two frames.  The lifter runs once over all test frames (p3d_serve) and the whole recurrence is
one VAE.filter_sequences call (k_vae_seq) -- no per-frame host round trip.

    python 3d_pose_vae_filter_kin.py --camera_frame --epochs 20 --cfg_file train.yml
    python 3d_pose_vae_filter_kin.py --evaluate --load 4874200 --lifter_dir DIR --linear_size 1024 \\
        --num_layers 2 --residual --batch_norm --camera_frame [--vae_weights W.npz]
"""
import importlib.util
import json
import os
import sys

import numpy as np

import predict_3dpose
from top_vae_3d_pose import data_handler, losses, models
from top_vae_3d_pose.args_def import ENVIRON as ENV, filter_samples

SEQ_LEN = 3
MAX_FRAMES = 1 << 20      # p3d_vae_seq_filter's N per call


def _base():
    """3d_pose_vae_filter.py (its name is no Python identifier): _lifter, lifter_flags, get_optimizer."""
    if "pose_vae_filter" not in sys.modules:
        spec = importlib.util.spec_from_file_location(
            "pose_vae_filter", os.path.join(os.path.dirname(os.path.abspath(__file__)), "3d_pose_vae_filter.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["pose_vae_filter"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["pose_vae_filter"]


def weights_path():
    return os.path.join(ENV.TRAIN_DIR, "vae_concat_seq", "last_model_weights")


def _factors(f):
    return (f.likelihood_factor, f.kcs_factor, f.dkl_factor)


def train(argv=None, read_from_config=False):
    """Epoch loop of 3d_pose_vae_filter_kin.py:158-280.  Returns (model, history) with history the
    per-epoch lists loss_train, loss_test (3-vectors), pred_error, error_34, error_3_pred and
    error_2_pred."""
    import torch
    f = ENV.setup(read_from_config=read_from_config, argv=argv)
    base = _base()
    d = predict_3dpose.load_data(base.lifter_flags(f))
    data_train, data_test = data_handler.load_dataset_3d_seq(d, seq_len=SEQ_LEN)
    size = data_train["frames"].shape[1]
    print("Dataset dims")
    print((len(data_train["starts"]), SEQ_LEN, size), (len(data_train["starts"]), size))
    print((len(data_test["starts"]), SEQ_LEN, size), (len(data_test["starts"]), size))
    B = f.batch_size
    K = filter_samples(f)
    model = models.VAE(SEQ_LEN * size, latent_dim=f.latent_dim, enc_dim=f.enc_dim, dec_dim=f.dec_dim,
                       human_3d_size=size, max_batch=max(B, 4096), seed=f.seed)
    optimizer = base.get_optimizer()
    print("Trainable weights:", len(model.param_table))
    print("Plots, sample images, progress bars and TF2 checkpoints are left out of this build")
    dev = model.device
    cols = torch.arange(SEQ_LEN * size, device=dev)

    def on_device(split):
        fr = torch.from_numpy(split["frames"]).to(dev)
        return fr, torch.from_numpy(split["starts"]).to(dev)

    def gather(fr, starts):
        """x [n, seq_len * size]: the windows' contiguous floats; y [n, size]: their last frames."""
        return fr.view(-1)[(starts * size)[:, None] + cols[None, :]], fr[starts + (SEQ_LEN - 1)]

    fr_tr, st_tr = on_device(data_train)
    fr_te, st_te = on_device(data_test)
    X_te, Y_te = gather(fr_te, st_te)
    nb_tr, nb_te = len(st_tr) // B, len(st_te) // B      # (the reference's floor: a short last batch is dropped)
    hist = {k: [] for k in ("loss_train", "loss_test", "pred_error", "error_34", "error_3_pred", "error_2_pred")}
    for epoch in range(1, f.epochs + 1):
        print("\nStarting epoch:", epoch)
        order = torch.from_numpy(np.random.permutation(len(st_tr))).to(dev)
        if f.device_noise and len(st_tr):      # the windows read in place and noised in one launch: no host copy
            so = st_tr[order]
            X = data_handler.add_noise_device(fr_tr, f.noise_3d, starts=so, width=SEQ_LEN * size, seed=f.seed, ctr=epoch)
            Y = fr_tr[so + (SEQ_LEN - 1)]
        else:
            X, Y = gather(fr_tr, st_tr[order])
            X = torch.from_numpy(data_handler.add_noise(X.cpu().numpy(), f.noise_3d)).to(dev)
        step_losses = torch.zeros((max(nb_tr, 1), 3), dtype=torch.float32, device=dev)
        for step in range(nb_tr):
            model.train_step_device(X[step * B:(step + 1) * B], Y[step * B:(step + 1) * B], _factors(f),
                                    optimizer.learning_rate, loss_out=step_losses[step])
            if step % f.step_log == 0:
                print(" Training loss at step %d: %.4f" % (step, float(step_losses[step].mean().item())))
                print(" Seen : %s samples" % ((step + 1) * B))
        hist["loss_train"].append(step_losses[:nb_tr].double().mean(dim=0).cpu().numpy())
        print("Evaluation on Test data...")
        lt = torch.zeros((max(nb_te, 1), 3), dtype=torch.float32, device=dev)
        errs = {k: [] for k in ("pred_error", "error_34", "error_3_pred", "error_2_pred")}
        for step in range(nb_te):
            xb, yb = X_te[step * B:(step + 1) * B], Y_te[step * B:(step + 1) * B]
            lt[step].copy_(losses.ELBO.compute_loss(model, xb, yb))
            preds = model(xb, training=False) if K is None else model(xb, training=False, samples=K)
            errs["pred_error"].append(losses.ELBO.compute_pred_error(yb, preds))
            errs["error_34"].append(losses.ELBO.compute_pred_error(xb[:, size:2 * size], yb))
            errs["error_3_pred"].append(losses.ELBO.compute_pred_error(xb[:, size:2 * size], preds))
            errs["error_2_pred"].append(losses.ELBO.compute_pred_error(xb[:, :size], preds))
        hist["loss_test"].append(lt[:nb_te].double().mean(dim=0).cpu().numpy())
        for k, v in errs.items():
            hist[k].append(float(torch.stack(v).mean().item()) if v else float("nan"))
        print('Epoch: {}, Test set ELBO: {}'.format(epoch, hist["loss_test"][-1]))
        print('Epoch: {}, Error frame 2 vs 3: {}'.format(epoch, hist["error_34"][-1]))
        print('Epoch: {}, Prediction Error: {}'.format(epoch, hist["pred_error"][-1]))
        print('Epoch: {}, Error frame 2 vs pred: {}'.format(epoch, hist["error_3_pred"][-1]))
        print('Epoch: {}, Error frame 1 vs pred: {}'.format(epoch, hist["error_2_pred"][-1]))
    os.makedirs(os.path.dirname(weights_path()), exist_ok=True)
    model.save_weights(weights_path())
    with open(os.path.join(os.path.dirname(weights_path()), "train.cfg"), "w") as cfg:
        json.dump(vars(f), cfg)
    print("Weights saved:", weights_path() + ".npz")
    return model, hist


def evaluate(argv=None, read_from_config=False, eps_ctr=1):
    """The recurrent evaluation of 3d_pose_vae_filter_kin.py:285-361.  Returns a dict: per_key
    {key2d: (err 2d-3d, err vae)}, overall (the two means over all frames), noise (mean, std, min,
    max of the per-frame lifter error), and -- for whoever wants to check them -- the device
    tensors pred, target, ref, frame_err, the offsets seq_off and the eps counter used.
    With --filter_samples K > 1 every frame's refined pose is the mean of K samples (draw k at eps
    counter eps_ctr + k); the dict then also holds ref_var and per_key_var {key2d: mean of ref_var}."""
    import torch
    f = ENV.setup(read_from_config=read_from_config, argv=argv)
    K = filter_samples(f)
    base = _base()
    pose3d, lf = base._lifter(f)
    d = predict_3dpose.load_data(lf)
    size = models.HUMAN_3D_SIZE
    vae = models.VAE(SEQ_LEN * size, latent_dim=f.latent_dim, enc_dim=f.enc_dim, dec_dim=f.dec_dim,
                     seed=f.seed, device=pose3d.device.index)
    vae.load_weights(f.vae_weights or weights_path())
    keys2d = list(d["test_set_2d"].keys())
    xs, ys = [], []
    for key2d in keys2d:
        x_in = d["test_set_2d"][key2d]
        x_out = d["test_set_3d"][data_handler.get_key3d(key2d, f.camera_frame)]
        if len(x_in) != len(x_out):
            raise ValueError("evaluate: %s has %d 2D frames and %d 3D frames" % (key2d, len(x_in), len(x_out)))
        xs.append(np.asarray(x_in, np.float32))
        ys.append(np.asarray(x_out, np.float32))
    lens = np.array([len(x) for x in xs], np.int64)
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(seq_off[-1])
    dev = pose3d.device
    X = torch.from_numpy(np.concatenate(xs)).to(dev)
    target = torch.from_numpy(np.concatenate(ys)).to(dev)
    pred = pose3d.serve_device(X)                       # the lifter once over all test frames
    ref = torch.empty_like(pred)
    ref_var = None if K is None else torch.empty_like(pred)
    frame_err = torch.empty((N, 2), dtype=torch.float32, device=dev)
    seq_err = torch.empty((len(keys2d), 2), dtype=torch.float64, device=dev)
    a = 0
    while a < len(keys2d):                              # one call, unless the set exceeds a call's frames
        b = a + 1
        while b < len(keys2d) and seq_off[b + 1] - seq_off[a] <= MAX_FRAMES:
            b += 1
        lo, hi = int(seq_off[a]), int(seq_off[b])
        if hi - lo > MAX_FRAMES:
            raise ValueError("evaluate: sequence %s has more than %d frames" % (keys2d[a], MAX_FRAMES))
        if hi > lo and K is not None:
            o = vae.filter_sequences(pred[lo:hi], seq_off[a:b + 1] - lo, ctr=eps_ctr, eps_row0=lo, target=target[lo:hi],
                                     want=("ref", "ref_var", "frame_err", "seq_err"), samples=K)
            ref[lo:hi], frame_err[lo:hi], seq_err[a:b] = o["ref"], o["frame_err"], o["seq_err"]
            ref_var[lo:hi] = o["ref_var"]
        elif hi > lo:
            o = vae.filter_sequences(pred[lo:hi], seq_off[a:b + 1] - lo, ctr=eps_ctr, eps_row0=lo, target=target[lo:hi],
                                     want=("ref", "frame_err", "seq_err"))
            ref[lo:hi], frame_err[lo:hi], seq_err[a:b] = o["ref"], o["frame_err"], o["seq_err"]
        else:
            seq_err[a:b] = 0
        a = b
    se = seq_err.cpu().numpy()
    per_key, per_key_var = {}, {}
    for i, key2d in enumerate(keys2d):
        print("Subject: {}, action: {}, fname: {}".format(*key2d))
        m = se[i] / max(int(lens[i]), 1)
        per_key[key2d] = (float(m[0]), float(m[1]))
        print("Err 2d-3d: {}, VAE: {}".format(m[0], m[1]))
        if K is not None:      # how much of a refined coordinate is the draw: the mean variance over the K samples
            lo, hi = int(seq_off[i]), int(seq_off[i + 1])
            per_key_var[key2d] = float(ref_var[lo:hi].double().mean()) if hi > lo else 0.0
            print("VAE sample variance ({} samples): {}".format(K, per_key_var[key2d]))
    overall = tuple(float(v) for v in se.sum(axis=0) / max(N, 1))
    print("Pred error 2d to 3d:", overall[0])
    print("Pred error vae filter:", overall[1])
    e1 = frame_err[:, 0].double()
    noise = (float(e1.mean()), float(e1.std(unbiased=False)), float(e1.min()), float(e1.max()))
    for v in noise:
        print(v)
    pose3d.check_errors()
    extra = {} if K is None else {"ref_var": ref_var, "per_key_var": per_key_var, "samples": K}
    return {**extra, "per_key": per_key, "overall": overall, "noise": noise, "pred": pred, "target": target, "ref": ref,
            "frame_err": frame_err, "seq_off": seq_off, "keys": keys2d, "eps_ctr": eps_ctr, "vae": vae, "pose3d": pose3d}


def main():
    argv = sys.argv[1:]
    cfg = "--cfg_file" in " ".join(argv)
    ENV.setup(read_from_config=cfg, argv=argv)
    if ENV.FLAGS.evaluate:
        res = evaluate(argv, read_from_config=cfg)
        res["vae"].close()
        res["pose3d"].close()
    else:
        model, _ = train(argv, read_from_config=cfg)
        model.close()


if __name__ == "__main__":
    main()
