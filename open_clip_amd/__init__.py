"""open_clip_amd: MI355X-native (gfx950) CLIP training hot path behind open_clip's model / loss API.

Public surface (mirrors the reference names):
    create_model, NativeCLIP            <- open_clip.factory.create_model / open_clip.model.CLIP (force_image_size=, force_context_length= as the
                                           reference's; dynamic_img_size=True: the image tower takes calls at other image sizes)
    resize_pos_embed, resize_text_pos_embed
                                        <- open_clip.model.resize_pos_embed / resize_text_pos_embed: a checkpoint's position tables at another image
                                           size / context length, resampled on the device (ocn_pos_resample_fwd), rectangular grids included
    NativeClipLoss, NativeSigLipLoss    <- open_clip.loss.ClipLoss / SigLipLoss
    NativeDistillClipLoss               <- open_clip.loss.DistillClipLoss (create_task(args, model, dist_model=teacher): DistillCLIPTask)
    get_model_config, add_model_config  <- open_clip.factory.get_model_config / add_model_config
    create_task, create_loss            <- open_clip.factory.create_task / create_loss (the reference's task classes around the native losses)
    create_optimizer, OptimizerCfg      <- open_clip_train.optim.create_optimizer / OptimizerCfg (the reference's parameter groups around the native
                                           optimizers NativeAdamW, NativeNAdamW, NativeMuon: open_clip_amd.optim)
    NativeModelEma, setup_ema           <- timm.utils.ModelEmaV3 as open_clip.task.TrainingTask.setup_ema uses it (open_clip_amd.ema: one launch per update)
    get_clip_metrics, zero_shot_accuracy, paired_retrieval_ranks, label_ranks
                                        <- open_clip_train.metrics.get_clip_metrics / open_clip_train.zero_shot.accuracy (open_clip_amd.metrics)
"""
from .configs import add_model_config, get_model_config, list_models  # noqa: F401


def __getattr__(name):  # lazy: importing the package must not require torch.cuda / the shared library
    if name in ("create_model", "NativeCLIP", "resize_pos_embed", "resize_text_pos_embed"):
        from . import model
        return getattr(model, name)
    if name in ("NativeClipLoss", "NativeSigLipLoss", "NativeDistillClipLoss"):
        from . import loss
        return getattr(loss, name)
    if name in ("create_task", "create_loss"):
        from . import factory
        return getattr(factory, name)
    if name in ("get_clip_metrics", "zero_shot_accuracy", "paired_retrieval_ranks", "label_ranks"):
        from . import metrics
        return getattr(metrics, name)
    if name in ("NativeAdamW", "NativeNAdamW", "NativeMuon", "muon_param_groups", "create_optimizer", "OptimizerCfg"):
        from . import optim
        return getattr(optim, name)
    if name in ("NativeModelEma", "setup_ema"):
        from . import ema
        return getattr(ema, name)
    raise AttributeError(name)
