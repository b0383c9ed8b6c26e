"""The VAE pose filter on top of the frozen lifter (mirror of src/top_vae_3d_pose)."""
