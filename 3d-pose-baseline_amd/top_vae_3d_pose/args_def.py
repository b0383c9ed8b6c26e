"""FLAGS shared by the VAE filter's modules (src/top_vae_3d_pose/args_def.py): the reference's names
and defaults for every flag this build reads, plus ``reaload_from_config_file`` for a settings file
shaped like src/train.yml (sections of ``key: value`` pairs).  The reference's spelling is kept."""
import argparse
import os

BAR_FORMAT = '{l_bar}{bar:30}{r_bar}'


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--learning_rate", type=float, default=0.001, help="Learning rate")
    p.add_argument("--dropout", type=float, default=1, help="Dropout keep probability. 1 means no dropout")
    p.add_argument("--batch_size", type=int, default=64, help="Batch size to use during training")
    p.add_argument("--epochs", type=int, default=200, help="How many epochs we should train for")
    p.add_argument("--camera_frame", action='store_true', default=False, help="Convert 3d poses to camera coordinates")
    p.add_argument("--batch_norm", action='store_true', default=False, help="Use batch_normalization")
    p.add_argument("--predict_14", action='store_true', default=False, help="predict 14 joints")
    p.add_argument("--use_sh", action='store_true', default=False, help="Use 2d pose predictions from StackedHourglass")
    p.add_argument("--action", type=str, default="All", help="The action to train on. 'All' means all the actions")
    p.add_argument("--optimizer", type=str, default="adam", help="Optimizer to use [adam, rmsprop]")
    p.add_argument("--model", type=str, default='VAE', help="Model to use: [VAE], default VAE.")
    p.add_argument("--latent_dim", type=int, default=24, help="VAE latent dimension")
    p.add_argument("--enc_dim", type=int, nargs='+', default=[40, 32], help="VAE encoder dimension")
    p.add_argument("--dec_dim", type=int, nargs='+', default=[32, 40], help="VAE decoder dimension")
    p.add_argument("--step_log", type=int, default=1000, help="Steps between training-loss lines")
    p.add_argument("--likelihood_factor", type=float, default=1.0, help="Term to regularize the likelihood loss for ELBO")
    p.add_argument("--dkl_factor", type=float, default=1.0, help="Term to regularize the likelihood loss for ELBO")
    p.add_argument("--kcs_factor", type=float, default=1.0, help="Term to regularize the likelihood loss for ELBO")
    # the bones loss's factors: the reference reads them from src/train.yml alone (losses.py:143-152)
    p.add_argument("--mag_factor", type=float, default=1.0, help="Term to regularize the bone-length loss")
    p.add_argument("--cos_factor", type=float, default=1.0, help="Term to regularize the direction-cosine loss")
    p.add_argument("--ang_factor", type=float, default=1.0, help="Term to regularize the angle (Gram matrix) loss")
    p.add_argument("--bones_mapping_dir", type=str, default="src/bones_mapping.yml",
                   help="File with the bones mapping (the built-in skeleton when the driver is not given one)")
    p.add_argument("--max_norm", action='store_true', default=False, help="Apply maxnorm constraint to the weights")
    p.add_argument("--residual", action='store_true', default=False,
                   help="Whether to add a residual connection every 2 layers")
    p.add_argument("--train_all", action='store_true', default=False, help="Train all the nn or only the vae nn")
    p.add_argument("--cameras_path", type=str, default="data/h36m/cameras.h5", help="Directory to load camera parameters")
    p.add_argument("--data_dir", type=str, default="data/h36m/", help="Data directory")
    p.add_argument("--train_dir", type=str, default="experiments", help="Training directory.")
    p.add_argument("--cfg_file", type=str, default="src/train.yml",
                   help="Config file, the values passed through args are remplaced by the specified in the file")
    p.add_argument("--sample", action='store_true', default=False, help="Set to True for sampling.")
    p.add_argument("--noised_sample", action='store_true', default=False,
                   help="Set to True for generate a sample of data with noise.")
    p.add_argument("--load", type=int, default=0, help="Try to load a previous checkpoint.")
    p.add_argument("--verbose", type=int, default=2, help="0:Error, 1:Warning, 2:INFO*(default), 3:debug")
    p.add_argument("--noise_3d", type=float, nargs=2, default=[1, 1],
                   help="Noise added for 3d points, second value is a noise added over a single joint")
    p.add_argument("--evaluate", action='store_true', default=False, help="Set to True for evaluating.")
    p.add_argument("--use_effb1", action='store_true', default=False,
                   help="Use Efficient Net B1 instead of B0 (accepted and ignored: the features are read "
                        "precomputed, whatever model made them)")
    p.add_argument("--effnet_outputs_path", type=str, default="data/human36m_effnet.hdf5",
                   help="File path for the outputs of the efficientNet model (.hdf5, or an .npz archive whose "
                        "member names are the dataset paths)")
    # build-specific: where evaluate() of 3d_pose_vae_filter_kin.py reads the filter's weights
    p.add_argument("--vae_weights", type=str, default=None,
                   help="The .npz of VAE weights that --evaluate loads (default: the one train() saves)")
    # build-specific: the frozen lifter (the reference hard-codes PoseBase and its checkpoint path)
    p.add_argument("--linear_size", type=int, default=1024, help="Lifter: size of each model layer")
    p.add_argument("--num_layers", type=int, default=2, help="Lifter: number of two_linear blocks")
    p.add_argument("--lifter_dir", type=str, default=None,
                   help="Lifter: the directory holding checkpoint-<load> (a predict_3dpose.train run's directory)")
    p.add_argument("--seed", type=int, default=0, help="Weight / eps / device-noise seed")
    # build-specific: 3d_pose_vae_filter_kin.py draws an epoch's noise on the device (data_handler.add_noise_device)
    p.add_argument("--device_noise", action='store_true', default=False,
                   help="Temporal filter: noise an epoch's windows on the GPU instead of through the host")
    # build-specific: the numbers behind gen_sample_img's picture (top_vae_3d_pose/samples.py)
    p.add_argument("--samples_dir", type=str, default="",
                   help="vae_filter.py: write each epoch's sample set (real, noised, predicted poses) to "
                        "DIR/samples_<epoch>.npz; empty (the default): off")
    # build-specific: the VAE output of the test blocks (and of --evaluate's recurrence) as the mean of K
    # posterior samples formed inside one launch (VAE.forward_device / filter_sequences, samples=K)
    p.add_argument("--filter_samples", type=int, default=1,
                   help="Posterior samples averaged into the VAE output at test time (1, the default: one draw, "
                        "as the reference)")
    return p


def filter_samples(flags):
    """--filter_samples checked: None at 1 (the callers then call what they call without the flag), else K."""
    k = int(getattr(flags, "filter_samples", 1))
    if not 1 <= k <= 64:
        raise ValueError("--filter_samples must be in 1 .. 64, got %d" % k)
    return None if k == 1 else k


class _ENV(object):
    def __init__(self):
        self.BAR_FORMAT = BAR_FORMAT
        self._parser = build_parser()
        self.FLAGS = self._parser.parse_args([])     # defaults until setup()
        self.TRAIN_DIR = None
        self.SUMMARIES_DIR = None

    def setup(self, read_from_config=False, argv=None):
        """Set the FLAGS (src/top_vae_3d_pose/args_def.py:112-137)."""
        self.FLAGS = self._parser.parse_args(argv)
        f = self.FLAGS
        self.TRAIN_DIR = os.path.join(f.train_dir, f.action, '{0}_top_model'.format(f.model),
                                      'dropout_{0}'.format(f.dropout),
                                      'epochs_{0}'.format(f.epochs) if f.epochs > 0 else '',
                                      'lr_{0}'.format(f.learning_rate), 'batch_size_{0}'.format(f.batch_size))
        self.SUMMARIES_DIR = os.path.join(self.TRAIN_DIR, "log")
        if read_from_config:
            self.reaload_from_config_file()
        return self.FLAGS

    def reaload_from_config_file(self):
        """Read the config file into FLAGS: every key of every section (args_def.py:139-146)."""
        import yaml
        with open(self.FLAGS.cfg_file) as fyml:
            cfg = yaml.safe_load(fyml)
        for _, data in (cfg or {}).items():
            for key, value in data.items():
                setattr(self.FLAGS, key, value)


ENVIRON = _ENV()
