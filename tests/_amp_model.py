"""Pure-Python model of the device-side loss-scale state machine (upf_loss_scale_update, csrc/optim.hip): what the kernel must
do, written from the contract in include/upflow_hip.h and not from the kernel — torch.amp.GradScaler.update with a floor of 1."""


class ScaleModel():
    def __init__(self, scale=2.0 ** 16, growth_interval=2000, growth_factor=2.0, backoff_factor=0.5, dynamic=True):
        self.scale, self.tracker, self.skipped, self.steps = float(scale), 0, 0, 0
        self.growth_interval, self.growth_factor, self.backoff_factor, self.dynamic = growth_interval, growth_factor, backoff_factor, dynamic

    def update(self, found_nonfinite):
        """One optimizer step whose gradients held (True) or did not hold (False) a NaN / inf; -> (S, tracker, skipped)."""
        if found_nonfinite:
            self.skipped += 1                                  # the step is skipped and counted in either mode
            if self.dynamic:
                self.scale = max(self.scale * self.backoff_factor, 1.0)
                self.tracker = 0
        else:
            self.steps += 1                                    # Adam's step counter advances on applied steps only
            if self.dynamic:
                self.tracker += 1
                if self.tracker == self.growth_interval:
                    self.scale *= self.growth_factor
                    self.tracker = 0
        return self.state()

    def state(self):
        return (self.scale, self.tracker, self.skipped)


def run(pattern, **kw):
    """pattern: iterable of booleans (True = a non-finite step) -> the list of (S, tracker, skipped) after each step."""
    m = ScaleModel(**kw)
    return [m.update(bool(bad)) for bad in pattern]
