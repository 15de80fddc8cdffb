from .sgd import FlatSGD
from .adam import FlatAdam
from .lars import FlatLARS
from .schedule import LRSchedule, HostLR

__all__ = ['FlatSGD', 'FlatAdam', 'FlatLARS', 'LRSchedule', 'HostLR',
           'schedule_from_config', 'build_optimizer']


def schedule_from_config(cfg) -> LRSchedule:
    """--lr / --lr-schedule / --warmup-steps / --lr-decay-steps /
    --lr-decay-gamma over --max-steps."""
    return LRSchedule(cfg.lr, getattr(cfg, 'lr_schedule', 'constant'),
                      total_steps=max(int(cfg.max_steps), 1),
                      warmup_steps=getattr(cfg, 'warmup_steps', 0),
                      decay_steps=getattr(cfg, 'lr_decay_steps', 0),
                      gamma=getattr(cfg, 'lr_decay_gamma', 0.1))


def build_optimizer(cfg, master_w, flat, name=None):
    """(optimizer, host_lr) for --optimizer on the f32 master buffer of the
    FlatSpace `flat`. host_lr is a HostLR to tick() before every logical step
    on the eager paths, or None: FlatLARS reads its schedule on the device,
    and a constant schedule without warmup never touches optimizer.lr."""
    name = name or getattr(cfg, 'optimizer', 'sgd')
    wd = getattr(cfg, 'weight_decay', 0.0)
    start = getattr(cfg, 'resume_step', 0) or 0
    sched = schedule_from_config(cfg)
    if name == 'lars':
        opt = FlatLARS(master_w, flat.segments(), sched,
                       momentum=cfg.momentum, weight_decay=wd,
                       eta=getattr(cfg, 'lars_eta', 1e-3), start_step=start)
        return opt, None
    if name == 'adam':
        opt = FlatAdam(master_w, lr=cfg.lr, weight_decay=wd)
    elif name == 'sgd':
        opt = FlatSGD(master_w, lr=cfg.lr, momentum=cfg.momentum,
                      weight_decay=wd)
    else:
        raise ValueError(f"unknown optimizer {name!r}")
    return opt, (None if sched.is_constant else HostLR(opt, sched, start))
