import sys, os, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubresnet_amd.models.ub_uresnet import UResNet
from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
from ubresnet_amd.training import epoch
from ubresnet_amd.optim import FlatAdam
from ubresnet_amd.staging import BatchStager
from ubresnet_amd import synthetic
from ubresnet_amd.augment import Augment
from ubresnet_amd.pixel_weights import PixelWeights
from ubresnet_amd.ema import ParamEMA
from ubresnet_amd.bnguard import StatsGuard
augment = Augment() if "--augment" in sys.argv else None      # python tools/soak.py [--augment] [--weights] [--detector] [--ema] [--accumulate K] [--stats-guard] [--focal GAMMA] [--normalize MODE] [--dice LAMBDA [--tversky A B]]
weights = PixelWeights(num_classes=3, radius=1, gain=2.0) if "--weights" in sys.argv else None
from ubresnet_amd.detector import DetectorEffects
detector = DetectorEffects(dead_runs=(0, 3), run_len=(1, 32), gain=(0.9, 1.1), noise_sigma=1.5, dead_label=0, dead_weight=0.0, seed=1) if "--detector" in sys.argv else None   # --detector: up to three runs of 1..32 dead wires per image, a gain in [0.9, 1.1], noise of sigma 1.5 on lit pixels; a dead pixel is background of weight 0
class NoWeight(object):                                        # --weights: the wire carries no weight entry, the device makes the weights
    def __init__(self, inner): self.inner = inner
    def __getitem__(self, idx): return {k: v for k, v in self.inner[idx].items() if not k.startswith("weight_")}
dev = torch.device("cuda:0"); torch.manual_seed(0)
model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev); model.compute_dtype = torch.bfloat16
focal = float(sys.argv[sys.argv.index("--focal") + 1]) if "--focal" in sys.argv else None   # --focal GAMMA: PixelWiseFocalLoss(gamma=GAMMA) instead of PixelWiseNLLLoss
normalize = sys.argv[sys.argv.index("--normalize") + 1] if "--normalize" in sys.argv else "pixels"   # --normalize pixels|valid|weights: the mean's denominator (implies the focal criterion, gamma 0 unless --focal is given)
if focal is not None or "--normalize" in sys.argv:
    from ubresnet_amd.training import PixelWiseFocalLoss
    crit = PixelWiseFocalLoss(gamma=focal if focal is not None else 0.0, normalize=normalize)
else: crit = PixelWiseNLLLoss()
if "--dice" in sys.argv:                                       # --dice LAMBDA [--tversky A B]: NLL (or the chosen focal) + LAMBDA * PixelWiseDiceLoss(alpha=A, beta=B), 0.5 0.5 without --tversky
    from ubresnet_amd.training import PixelWiseDiceLoss, WeightedSumLoss
    ab = [float(v) for v in sys.argv[sys.argv.index("--tversky") + 1:sys.argv.index("--tversky") + 3]] if "--tversky" in sys.argv else [0.5, 0.5]
    crit = WeightedSumLoss([(1.0, crit), (float(sys.argv[sys.argv.index("--dice") + 1]), PixelWiseDiceLoss(alpha=ab[0], beta=ab[1]))])
opt = FlatAdam(model, lr=1e-3, weight_decay=1e-4)
ema = ParamEMA(opt, decay=0.999, warmup=10) if "--ema" in sys.argv else None   # --ema: averaged weights, updated after every step
sg = StatsGuard(model, optimizer=opt) if "--stats-guard" in sys.argv else None   # --stats-guard: BatchNorm statistics committed or restored after every step (the optimizer here is unguarded: the scan alone decides)
accumulate = int(sys.argv[sys.argv.index("--accumulate") + 1]) if "--accumulate" in sys.argv else 1   # --accumulate K: one optimizer step per K batches (GradAccumulator); 300 steps are then 300 * K batches
ld = synthetic.SyntheticLArCVDataset(height=512, width=512, tag="train", nentries=64, cache=64); ld.start(16)
if weights is not None: ld = NoWeight(ld)
def stager():
    if "--event-crops" not in sys.argv: return BatchStager(ld, 16, 512, 512, tag="train", augment=augment, weights=weights, detector=detector)
    from ubresnet_amd import crops                              # --event-crops: 16 crops of 512 x 512 per batch cut on the device from eight pinned synthetic 3 x 1008 x 3456 events (EventCropStager; --augment does not apply, flips come from the cropper)
    events = [crops.LabelledEvent(*(torch.from_numpy(a).pin_memory() for a in synthetic.make_labelled_event(3, 1008, 3456, 5000 + 10 * i))) for i in range(8)]
    return crops.EventCropStager(events, crops.EventCropper(crop=(512, 512), per_event=16, min_lit=2000, tries=8, flip_rows=True, flip_cols=True, seed=1), weights=weights, detector=detector)
t0 = time.perf_counter()
with stager() as st:
    for ep in range(6):
        loss, acc = epoch.train(st, model, crit, opt, 50 * accumulate, iiter=ep, print_freq=25 * accumulate, accumulate=accumulate, stats_guard=sg, ema=ema)
        print(ep, round(loss, 4), "mem GB %.2f" % (torch.cuda.max_memory_allocated() / 2**30), "acc[1] %.1f" % acc, st.stage_times() if hasattr(st, "stage_times") else "", flush=True)
torch.cuda.synchronize(); print("%d steps (%d batches) in %.1f s; finite params: %s" % (opt.steps, 300 * accumulate, time.perf_counter() - t0, all(torch.isfinite(p).all().item() for p in model.parameters())))
if ema is not None: print("ema updates %d held %d; finite average: %s" % (ema.updates, ema.held, bool(torch.isfinite(ema.shadow).all())))
if hasattr(crit, "gamma"): print("criterion: gamma %g, normalize %s, last batch %s" % (crit.gamma, crit.normalize, crit.read()))
elif hasattr(crit, "read"): print("criterion: weights %s, last batch %s" % (crit.weights, crit.read()))
if sg is not None: print("stats guard: %s; finite statistics: %s" % (sg.read(), all(torch.isfinite(b).all().item() for b in model.buffers() if b.is_floating_point())))
