#!/usr/bin/env python3
"""Cluster the event products of synthetic labelled events on the device and print the cluster table, largest first.

    python tools/cluster_events.py [--events N] [--rows R] [--cols C] [--top K] [--min-pixels M] [--connectivity 4|8] [--by-class]
                                   [--moments] [--adc-scale S] [--truth] [--match-planes] [--match-threshold T]

Every event goes through WholeViewSegmenter(output="products") and an EventClusterer (ubresnet_amd/clusters.py); nothing leaves
the device until Clusters.read(), which copies the count and that many table rows.  The model has seeded random weights, so the
classes mean nothing here; `shower` is the share of class --shower-class among the cluster's pixels.  With --moments a
ClusterMoments (ubresnet_amd/shapes.py) runs behind the clusterer and the table gains the cluster's charge (summed ADC), the share
of the shower class in that charge, its length (2 sqrt 3 times the major extent: exact for a uniform line), width and linearity.
With --truth the truth of the event is clustered the same way (overlap.truth_products into a second EventClusterer) and a
ClusterOverlap (ubresnet_amd/overlap.py) matches the predicted clusters against the true ones: beside the table above, per
predicted cluster, largest first, its purity, the efficiency of its best match and that match, pixel- and charge-weighted, and the
event's adjusted Rand index.  (Without --by-class both sides cluster the same lit pixels whatever their class, and agree.)
With --match-planes the events are synthetic.make_matched_event -- the same objects seen by every plane -- and a PlaneMatcher
(ubresnet_amd/planes.py) runs behind the clusterer: the clusters of at least --min-pixels pixels are matched across the planes by
their time profiles, and the mutually best pairs at or above --match-threshold (containment) and the triples are printed with the
object most pixels of each cluster belong to.  (--planes is the number of planes, as before.)"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=2)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--cols", type=int, default=832)
    ap.add_argument("--planes", type=int, default=3)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--shower-class", type=int, default=2)
    ap.add_argument("--top", type=int, default=12)
    ap.add_argument("--min-pixels", type=int, default=4)
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    ap.add_argument("--by-class", action="store_true")
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--moments", action="store_true")
    ap.add_argument("--adc-scale", type=int, default=16)
    ap.add_argument("--truth", action="store_true")
    ap.add_argument("--match-planes", action="store_true")
    ap.add_argument("--match-threshold", type=float, default=0.5)
    ap.add_argument("--slots", type=int, default=512)
    a = ap.parse_args()
    import torch
    from ubresnet_amd import clusters, deploy, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("cluster_events: needs a ROCm device; the HIP path has no CPU fallback")
    torch.manual_seed(7)
    model = deploy.load_model(None, "cuda:0", num_classes=a.classes)
    seg = deploy.WholeViewSegmenter(model, rows=a.rows, cols=a.cols, planes=a.planes, tile=(min(512, a.rows), min(832, a.cols)), batch=3,
                                    dtype=torch.float16, output="products")
    cl = clusters.EventClusterer(a.planes, a.rows, a.cols, a.classes, a.connectivity, a.by_class, 255, a.capacity, "cuda:0")
    cm = None
    if a.moments:
        from ubresnet_amd import shapes
        cm = shapes.ClusterMoments(cl, adc_scale=a.adc_scale)
    if a.truth:
        from ubresnet_amd import overlap
        cl_true = clusters.EventClusterer(a.planes, a.rows, a.cols, a.classes, a.connectivity, a.by_class, 255, a.capacity, "cuda:0")
        co = overlap.ClusterOverlap(a.planes, a.rows, a.cols, 4 * a.capacity, None, a.adc_scale, "cuda:0")
    pm = None
    if a.match_planes:
        from ubresnet_amd import planes
        pm = planes.PlaneMatcher(cl, a.slots, max(a.min_pixels, 1), 1, None, a.adc_scale)
    for e in range(a.events):
        if pm:
            image, truth, instance = synthetic.make_matched_event(a.planes, a.rows, a.cols, 1000 + 10 * e)
        else:
            image, truth = synthetic.make_labelled_event(a.planes, a.rows, a.cols, 1000 + 10 * e)
        view = torch.from_numpy(image[:, None].copy()).cuda()
        found = cl(seg(view))
        matches = pm(found, view) if pm else None                 # launched before anything is read back
        if a.truth:                                               # launched before anything is read back
            ov = co(found, cl_true(*overlap.truth_products(torch.from_numpy(truth).cuda(), view)), view)
        shape = cm(found, view).read(min_pixels=a.min_pixels) if cm else None
        tab = shape.clusters if cm else found.read(min_pixels=a.min_pixels)
        order = torch.argsort(tab.pixels, descending=True)[:a.top]
        frac, mean = tab.fractions(), tab.mean_confidence()
        print("event %d: %d clusters, %d of at least %d pixels; foreign labels so far %d"
              % (e, tab.total, len(tab), a.min_pixels, int(found.status.item())))
        more = ""
        if cm:
            charge, qfrac, length, width, lin = shape.charge(), shape.charge_fractions(), shape.length(), shape.width(), shape.linearity()
            more = "  %10s  %8s  %7s  %6s  %9s" % ("charge", "shower q", "length", "width", "linearity")
        print("  plane  pixels  rows        cols        shower  mean confidence" + more)
        for i in order.tolist():
            r0, r1, c0, c1 = tab.bbox[i].tolist()
            if cm:
                more = "           %10.1f  %8.3f  %7.1f  %6.1f  %9.4f" % (float(charge[i]), float(qfrac[i, a.shower_class]), float(length[i]),
                                                                           float(width[i]), float(lin[i]))
            print("  %5d  %6d  %4d..%-4d  %4d..%-4d  %6.3f  %.4f" % (int(tab.plane[i]), int(tab.pixels[i]), r0, r1, c0, c1,
                                                                  float(frac[i, a.shower_class]), float(mean[i])) + more)
        if pm:
            mt = matches.read()
            ids, inst = found.ids.cpu(), torch.from_numpy(instance)
            obj = []
            for k in mt.cluster.tolist():                             # the object most pixels of the cluster belong to
                of = inst[ids == k]
                obj.append(int(torch.bincount(of[of >= 0]).argmax()) if bool((of >= 0).any()) else -1)
            pairs = mt.matched(a.match_threshold)
            print("  %d candidates of at least %d pixels, %d pairs share a time bin, %d matched at containment >= %.2f; %d pixels dropped"
                  % (len(mt), pm.min_pixels, len(mt.pairs()), len(pairs), a.match_threshold, mt.dropped))
            iou, tio = mt.charge_iou(), mt.time_iou()
            print("  cluster (plane, object)  cluster (plane, object)  containment  charge iou  time iou")
            for i, j, v in pairs[:a.top]:
                print("  %7d (%d, %3d)         %7d (%d, %3d)         %11.3f  %10.3f  %8.3f"
                      % (int(mt.cluster[i]), int(mt.plane[i]), obj[i], int(mt.cluster[j]), int(mt.plane[j]), obj[j], v, iou[(i, j)], tio[(i, j)]))
            triples = mt.triples(a.match_threshold)
            print("  %d triples: %s" % (len(triples), ", ".join("(%s) of objects (%s)" % (", ".join(str(int(mt.cluster[c])) for c in t),
                                                                                       ", ".join(str(obj[c]) for c in t)) for t in triples[:a.top])))
        if a.truth:
            match = ov.read()
            sizes, eff_of = match.sizes_a(), {}
            for weighted in (False, True):
                eff = match.efficiency(weighted)
                eff_of[weighted] = dict(zip(eff.cluster.tolist(), eff.value.tolist()))
            pur = {w: match.purity(w) for w in (False, True)}
            print("  %d pairs of %d predicted and %d true clusters; adjusted Rand index %.4f" % (len(match), len(sizes), len(match.sizes_b()), match.ari()))
            print("  cluster  pixels  purity  efficiency  best true  |  by charge: purity  efficiency  best true")
            for k in sorted(sizes, key=lambda c: -sizes[c])[:a.top]:
                cells = []
                for weighted in (False, True):
                    i = pur[weighted].cluster.tolist().index(k)
                    best = int(pur[weighted].best[i])
                    cells += [float(pur[weighted].value[i]), eff_of[weighted].get(best, float("nan")), best]
                print("  %7d  %6d  %6.3f  %10.3f  %9d  |  %17.3f  %10.3f  %9d" % ((k, sizes[k]) + tuple(cells)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
