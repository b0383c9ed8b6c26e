"""Losses of the VAE filter (src/top_vae_3d_pose/losses.py:12-57) on the device."""
import _p3d
from top_vae_3d_pose.args_def import ENVIRON as ENV


def _mse(a, b):
    """mean((a - b)^2) of two device tensors of one shape through p3d_mse (k_mse); a device scalar."""
    import torch
    if a.shape != b.shape or a.dim() != 2:
        raise ValueError("mse: expected two [B, D] tensors of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    a, b = a.contiguous().float(), b.contiguous().float()
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    _p3d.check(_p3d.lib().p3d_mse(_p3d.ptr(a), _p3d.ptr(b), a.shape[0], a.shape[1], _p3d.ptr(out), None,
                                  _p3d.stream_handle()), "p3d_mse")
    return out[0]


def _factors():
    f = ENV.FLAGS
    return (f.likelihood_factor, f.kcs_factor, f.dkl_factor)


def _bones_factors():
    f = ENV.FLAGS
    return (f.mag_factor, f.cos_factor, f.dkl_factor, f.ang_factor)


def loss_bones(model, inputs, targets, eps=None):
    """The bones loss (losses.py:113-156): the device 4-vector [MAG, COS, DKL, ANG] under FLAGS'
    factors -- one launch; the tensor is the model's loss buffer.  `model` is a VAEBones, `targets`
    the [B, 64] bones tensor [mag | cos] or the reference's (magnitudes, dir_cos) pair."""
    if isinstance(targets, (tuple, list)):
        import torch
        targets = torch.cat([torch.as_tensor(targets[0]), torch.as_tensor(targets[1])], dim=1)
    model._calls += 1
    return model.loss_device(inputs, targets, _bones_factors(), eps=eps, ctr=model._calls)


class ELBO():
    @classmethod
    def compute_loss(cls, model, inputs, targets, eps=None):
        """ELBO: the device 3-vector [likelihood, KCS, KL] under FLAGS' factors (losses.py:14-40) --
        one launch; the tensor is the model's loss buffer (copy it to keep it across calls)."""
        model._calls += 1
        return model.loss_device(inputs, targets, _factors(), eps=eps, ctr=model._calls)

    @classmethod
    def compute_error_3d_vs_vae(cls, real_out, out_3d, out_vae):
        """MSE of real vs out_3d and of real vs out_vae (losses.py:43-49), device scalars."""
        return _mse(real_out, out_3d), _mse(real_out, out_vae)

    @classmethod
    def compute_pred_error(cls, real_out, pred_out):
        """MSE between the predictions and the targets (losses.py:52-56)."""
        return _mse(real_out, pred_out)
