"""Train the bones filter over [x2d | bone lengths | direction cosines | effnet_out] on top of the
frozen 2D->3D lifter (src/pose_3d_bones.py): the 1376-input VAEBones of models.py:485-573 built
with use_2d=True, use_effnet_ouptut=True, pred_bones=True, trained on losses.loss_bones.

train() is the reference's epoch loop (:174-320) in the style of 3d_pose_effnet_2d_vae_filter.py:
the frozen lifter comes from --load / --lifter_dir, X / Y are built in key order, the precomputed
EfficientNet features are loaded ONCE onto the device and indexed in place by the epoch's
permutation, and the targets are converted to bones ONCE per split on the device (the float64
arithmetic of bones.convert_to_bones, data_handler's pred_bones) and gathered per epoch.  A step
is p3d_serve, the float32 conversion of the lifter's output (:162-165, convert_to_bones_tf) and
one train_step_device([x, bones, (F, idx)]).

Evaluation (:257-283) is lifter -> float64-arithmetic bones -> filter -> convert_to_joints of the
prediction and of the target bones -> the two mean-square errors.  The reference hands a float64
target and a float32 lifter output to one tf.square and would not run as written; here out_3d is
widened and both errors are formed in float64.  The test split's loss_bones vector is recorded as
well (the reference has it commented out).  Plots, gen_sample_img, tqdm and the TF2 checkpoints
are left out; the weights are saved as an .npz under the Keras names in 3d_effnet_2d_vae_bones/.

    python pose_3d_bones.py --load 4874200 --lifter_dir DIR --linear_size 1024 --num_layers 2 --residual \\
        --batch_norm --camera_frame --epochs 20 --cfg_file train.yml --effnet_outputs_path effnet.npz
"""
import importlib.util
import json
import os
import sys

import predict_3dpose
from top_vae_3d_pose import bones, losses, models
from top_vae_3d_pose.args_def import ENVIRON as ENV, filter_samples

_HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


wide = _sibling("pose_effnet_2d_vae_filter", "3d_pose_effnet_2d_vae_filter.py")   # key order, the feature table
base = wide.base                                                                   # get_optimizer, the frozen lifter


def _factors():
    f = ENV.FLAGS
    return (f.mag_factor, f.cos_factor, f.dkl_factor, f.ang_factor)


def train_step_vae(model, x_data, y_bones, effnet, optimizer, loss_out=None, bones_buf=None):
    """One training step (pose_3d_bones.py:158-171): the device loss 4-vector [MAG, COS, DKL, ANG].
    `y_bones` is the [B, 64] target, `effnet` a [B, effnet_size] tensor or (table, idx)."""
    out_3d = model.pose3d.serve_device(x_data)
    b64 = model.bones_tf(out_3d, out=bones_buf)
    return model.vae.train_step_device(model.segments(x_data, b64, effnet), y_bones, _factors(),
                                       optimizer.learning_rate, loss_out=loss_out)


def _mse64(a, b):
    return ((a.double() - b.double()) ** 2).mean()


def train(argv=None, read_from_config=False):
    """Epoch loop of pose_3d_bones.py:174-320.  Returns (model, history) with history the per-epoch
    lists loss_train, loss_test (4-vectors), error_3d_out and error_vae_out."""
    import torch
    f = ENV.setup(read_from_config=read_from_config, argv=argv)
    if filter_samples(f) is not None:
        raise NotImplementedError("--filter_samples above 1 is not served by the bones filter: its outputs are lengths "
                                  "and direction cosines, and direction cosines do not average")
    if f.train_all:
        raise NotImplementedError("--train_all is not built: the lifter stays frozen")
    if f.sample:
        raise NotImplementedError("--sample (gen_sample_img) is matplotlib visualisation, not built")
    if f.use_effb1:
        print("--use_effb1 is accepted and ignored: the features are read precomputed from", f.effnet_outputs_path)
    optimizer = base.get_optimizer()
    bones_joints = None
    if os.path.isfile(f.bones_mapping_dir):      # (the built-in skeleton otherwise; another one is refused)
        bones_joints = bones.get_bones_joints(bones.get_bones_mapping(f.bones_mapping_dir))
    pose3d, lf = base._lifter(f)
    d = predict_3dpose.load_data(lf)
    dev = pose3d.device
    X, Y, F = wide._device_split(d, lf, "train", f.effnet_outputs_path, dev)
    Xt, Yt, Ft = wide._device_split(d, lf, "test", f.effnet_outputs_path, dev)
    Yb = bones.convert_to_bones(Y, bones_joints, precise=True)       # the targets, once per split
    Ytb = bones.convert_to_bones(Yt, bones_joints, precise=True)
    Ytj = bones.convert_to_joints(Ytb, bones_joints=bones_joints)    # (:279) the target bones walked back, float64
    model = models.Pose3DVaeBones(latent_dim=f.latent_dim, enc_dim=f.enc_dim, dec_dim=f.dec_dim, use_effnet_ouptut=True,
                                  use_2d=True, pose3d=pose3d, effnet_size=int(F.shape[1]),
                                  max_batch=max(f.batch_size, 4096), seed=f.seed)
    print("Training only VAE weights:", len(model.vae.param_table))
    print("Plots, sample images, progress bars and TF2 checkpoints are left out of this build")
    B = f.batch_size
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(f.seed))
    bones_buf = torch.empty((B, 64), dtype=torch.float32, device=dev)
    hist = {"loss_train": [], "loss_test": [], "error_3d_out": [], "error_vae_out": []}
    for epoch in range(1, f.epochs + 1):
        print("\nStarting epoch:", epoch)
        n = X.shape[0]
        nb = n // B
        perm = torch.randperm(n, device=dev, generator=gen)
        Xp, Ybp = X[perm], Yb[perm]        # one gather per epoch; the feature table stays where it is
        step_losses = torch.zeros((max(nb, 1), 4), dtype=torch.float32, device=dev)
        for step in range(nb):
            sl = slice(step * B, (step + 1) * B)
            train_step_vae(model, Xp[sl], Ybp[sl], (F, perm[sl]), optimizer, loss_out=step_losses[step],
                           bones_buf=bones_buf)
            if step % f.step_log == 0:
                mag, cos, dkl, ang = (float(v) for v in step_losses[step].cpu())
                print(" Losses:: MAG %.4f, COS %.4f, DKL %.4f, ANG %.4f" % (mag, cos, dkl, ang))
                print(" Training loss at step %d: %.4f" % (step, mag + cos + dkl + ang))
                print(" Seen : %s samples" % ((step + 1) * B))
        hist["loss_train"].append(step_losses[:nb].double().mean(dim=0).cpu().numpy())
        print("Evaluation on Test data...")
        nbt = Xt.shape[0] // B
        lt = torch.zeros((max(nbt, 1), 4), dtype=torch.float32, device=dev)
        e3, ev = [], []
        for step in range(nbt):
            sl = slice(step * B, (step + 1) * B)
            xb, fb = Xt[sl], Ft[sl]
            out_3d = model.pose3d.serve_device(xb)
            b64 = bones.convert_to_bones(out_3d, bones_joints, precise=True)
            segs = model.segments(xb, b64, fb)
            model.vae._calls += 1
            y = model.vae.forward_device(segs, ctr=model.vae._calls)["y"]
            lt[step].copy_(losses.loss_bones(model.vae, segs, Ytb[sl]))
            vae_joints = bones.convert_to_joints(y, bones_joints=bones_joints)
            e3.append(_mse64(Ytj[sl], out_3d))
            ev.append(_mse64(Ytj[sl], vae_joints))
        hist["loss_test"].append(lt[:nbt].double().mean(dim=0).cpu().numpy())
        hist["error_3d_out"].append(float(torch.stack(e3).mean().item()) if e3 else float("nan"))
        hist["error_vae_out"].append(float(torch.stack(ev).mean().item()) if ev else float("nan"))
        print('Epoch: {}, Test set loss [MAG, COS, DKL, ANG]: {}'.format(epoch, hist["loss_test"][-1]))
        print('Error real vs 3d out:', hist["error_3d_out"][-1])
        print('Error real vs vae out:', hist["error_vae_out"][-1])
    out_dir = os.path.join(ENV.TRAIN_DIR, "3d_effnet_2d_vae_bones")
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
