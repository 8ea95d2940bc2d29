"""get_model(args) as the reference's factory (modelFactory.py:6-29): the AERO generator or the Seanet baseline (`model: seanet`, inference) and, for `adversarial: true` experiments, the
critics of `discriminator_models`: the MelGAN multi-scale critic (`msd_melgan`, the critic of every aero experiment file) and the HiFi-GAN
multi-period critic (`mpd`, kwargs from `experiment.mpd`, the constructor's defaults when the block is absent), built msd_melgan first.
The critics `msd_hifi` / `hifi` (which the reference itself cannot run) raise NotImplementedError."""
from aero_amd.trainer import build_models as get_model  # noqa: F401
