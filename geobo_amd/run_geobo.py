"""YAML-driven workflow around the MI355X inversion -- the reference's `run_geobo.py:380-469` main flow as a function.

    python -m geobo_amd.run_geobo settings.yaml

read survey + drill data -> Inversion.cubing (GPU) -> six VTK cubes -> optional BO proposals.  Plotting (matplotlib /
pyvista) and the synthetic-model generator (`gen_simulation`) of the reference are not part of this package.
"""
import os
import sys

import numpy as np

from . import config_loader, dataio
from .acquisition import Acquisition
from .inversion import Inversion


def run(settings, method="auto", bayesopt=True, write=True):
    s = config_loader.load(settings, create_outpath=write)
    if getattr(s, "gen_simulation", False):
        print("gen_simulation is not supported here: using the existing input files")
    inv = Inversion(settings=s, method=method)
    voxelpos = inv.create_cubegeometry()
    # run_geobo.py:400-403 -- the reference re-shapes the centre arrays to (xN, yN, zN); flat order is unchanged
    for name in ("xxx", "yyy", "zzz"):
        setattr(inv, name, getattr(inv, name).reshape(s.xNcube, s.yNcube, s.zNcube))
    gravfield, magfield, sensor_locations = dataio.read_surveydata(s)
    drilldata, drillcoord, drillminmax = dataio.read_drilldata(s, s.drill_features, voxelpos)
    drilldata0 = drilldata[s.ifeature]
    drillfield = drilldata0[drilldata0 != 0]
    cubes = inv.cubing(gravfield, magfield, drillfield, sensor_locations, drilldata0)
    names = ["cube_density", "cube_magsus", "cube_drill", "cube_density_variance", "cube_magsus_variance", "cube_drill_variance"]
    if write:
        origin = (voxelpos[0].min(), voxelpos[1].min(), voxelpos[2].min())
        voxelsize = (s.xvoxsize, s.yvoxsize, s.zvoxsize)
        for c, n in zip(cubes, names):
            dataio.create_vtkcube(c, origin, voxelsize, fname=os.path.join(s.outpath, n + ".vtk"))
    updated = None
    more = getattr(s, "assimilate_drill", None)           # optional YAML key assimilate_drill: a further drill csv (in inpath, the format
    if more:                                              # of FNAME_drilldata) whose values are added WITHOUT a new step; every product
        import copy                                       # below then works from the extended factor
        s_more = copy.copy(s)
        s_more.FNAME_drilldata = str(more)
        extra = np.asarray(dataio.read_drilldata(s_more, s.drill_features, voxelpos)[0][s.ifeature]).reshape(-1)
        # (a voxel that carries a value already keeps it: one drill row per voxel)
        new_vox = np.flatnonzero((extra != 0) & (np.asarray(drilldata0).reshape(-1) == 0))
        if new_vox.size:
            updated = inv.assimilate_drill(new_vox, extra[new_vox])
            if write:
                for c, n in zip(updated, names):
                    dataio.create_vtkcube(c, origin, voxelsize, fname=os.path.join(s.outpath, n + "_updated.vtk"))
    dropped = None
    dd = getattr(s, "drop_data", None)                    # optional YAML key drop_data: {grav: [...], magn: [...], drill: [...]} -- stations
    if dd:                                                # and drill rows the model is to be shown WITHOUT: the scales
        dropped = inv.reweight_data(grav=dd.get("grav"), magn=dd.get("magn"), drill=dd.get("drill"), commit=True)      # are committed,
        if write:                                         # one step follows, and every product below works from the reduced system
            for c, n in zip(dropped["cubes"], names):
                dataio.create_vtkcube(c, origin, voxelsize, fname=os.path.join(s.outpath, n + "_dropped.vtk"))
    cv = getattr(s, "cross_validate", None)               # optional YAML key cross_validate: loo | holes | patches
    if cv:
        cv_result = inv.cross_validate(folds=str(cv), write=write)
    out = dict(zip(names, cubes), inversion=inv, drillcoord=drillcoord, inputs=(gravfield, magfield, drillfield, sensor_locations, drilldata0))
    if updated is not None:
        out.update({n + "_updated": c for n, c in zip(names, updated)}, assimilated_voxels=new_vox)
        cubes = updated                                   # (the proposals below look at the cubes with the new values in)
    if dropped is not None:
        out.update({n + "_dropped": c for n, c in zip(names, dropped["cubes"])}, dropped_data=dropped)
        cubes = dropped["cubes"]                          # (... and without the dropped rows)
    if cv:
        out["cross_validation"] = cv_result
    bm = getattr(s, "block_model", None)                  # optional YAML key block_model: [bx, by, bz] voxels per block
    if bm:
        out["block_model"] = inv.block_statistics(tuple(bm), write=write)
    pp = getattr(s, "predict_points", None)               # optional YAML key predict_points: csv (in inpath) with columns X, Y, Z
    if pp:
        import pandas as pd
        fname = pp if os.path.isabs(str(pp)) else os.path.join(s.inpath, str(pp))
        pts = pd.read_csv(fname)[["X", "Y", "Z"]].to_numpy(dtype=np.float64)
        out["points_prediction"] = inv.predict_points(pts)
        if write:
            inv._write_points_prediction(pts, out["points_prediction"])
    path = getattr(s, "predict_path", None)               # optional YAML key predict_path: [x0, y0, azimuth, dip] of a planned hole
    if path:
        out["path_prediction"] = inv.predict_path(*[float(v) for v in path])
        if write:
            inv._write_points_prediction(out["path_prediction"]["points"], out["path_prediction"], fname="path_prediction.csv")
    nsamp = int(getattr(s, "posterior_samples", 0) or 0)     # optional YAML keys posterior_samples (default 0) and sample_seed
    if nsamp > 0:
        samples = inv.sample_posterior(nsamp, seed=int(getattr(s, "sample_seed", 0) or 0))
        out["posterior_samples"] = samples
        if write:
            for c, n in zip(samples, ("density", "magsus", "drill")):
                for k in range(nsamp):
                    dataio.create_vtkcube(c[k], origin, voxelsize, fname=os.path.join(s.outpath, "cube_%s_sample_%03d.vtk" % (n, k)))
    def write_probability_cubes(cubes_p, prop, blk, tag):
        """One VTK cube per cutoff, cube_<property>_<tag>_<k>.vtk, at voxel or block support; nothing for None."""
        from .resources import PROPS, property_index
        size = voxelsize if blk is None else tuple(v * b for v, b in zip(voxelsize, blk))
        for k, cube in enumerate(cubes_p if cubes_p is not None else ()):
            dataio.create_vtkcube(cube, origin, size, fname=os.path.join(s.outpath, "cube_%s_%s_%d.vtk" % (PROPS[property_index(prop)], tag, k)))
    gt = getattr(s, "grade_tonnage", None)                # optional YAML key grade_tonnage: {cutoffs, property, samples, offset, block,
    if gt:                                                # voxel_probability}; sample_seed is shared with posterior_samples
        prop = gt.get("property", "drill")
        blk = tuple(gt["block"]) if gt.get("block") else None
        res = inv.grade_tonnage(list(gt["cutoffs"]), prop=prop, n=int(gt.get("samples", 256)), seed=int(getattr(s, "sample_seed", 0) or 0),
                                offset=float(gt.get("offset", 0.0)), block=blk, voxel_probability=bool(gt.get("voxel_probability", False)),
                                write=write)
        out["grade_tonnage"] = res
        if write and "probability" in res:
            write_probability_cubes(res["probability"], prop, blk, "exceed")
    gbd = getattr(s, "geobodies", None)                   # optional YAML key geobodies: {cutoffs, property, samples, offset, block,
    if gbd:                                               # neighbours, min_voxels, seeds: drill, probability}; sample_seed is shared
        prop = gbd.get("property", "drill")
        blk = tuple(gbd["block"]) if gbd.get("block") else None
        res = inv.geobodies(list(gbd["cutoffs"]), prop=prop, n=int(gbd.get("samples", 256)), seed=int(getattr(s, "sample_seed", 0) or 0),
                            offset=float(gbd.get("offset", 0.0)), block=blk, neighbours=int(gbd.get("neighbours", 6)),
                            min_voxels=int(gbd.get("min_voxels", 1)), seeds=gbd.get("seeds") or None,
                            probability=gbd.get("probability") or None, write=write)
        out["geobodies"] = res
        if write:
            # (one cube per cutoff: the seeded body's probability when asked for, else the largest body's)
            write_probability_cubes(res.get("probability_seeded", res.get("probability_largest")), prop, blk, "connected")
    dri = getattr(s, "drill_intercepts", None)            # optional YAML key drill_intercepts: {cutoffs, property, samples, offset,
    if dri:                                               # min_length, max_gap} (metres), optionally holes or paths (+ step)
        from .intercepts import parse_yaml
        kw, along = parse_yaml(dri)
        seed = int(getattr(s, "sample_seed", 0) or 0)     # (shared with posterior_samples)
        out["drill_intercepts"] = inv.drill_intercepts(seed=seed, write=write, **kw)
        if along:
            out["drill_intercepts_holes"] = inv.drill_intercepts(seed=seed, write=write, **kw, **along)
    ncamp = int(getattr(s, "drill_campaign", 0) or 0)    # optional YAML keys drill_campaign (q, default 0) and campaign_utility
    if ncamp > 0:
        out["drill_campaign"] = inv.propose_drill_campaign(ncamp, utility=getattr(s, "campaign_utility", None) or "information", write=write)
    if bayesopt:
        acq = Acquisition(s, cubes[2], cubes[5])
        if getattr(s, "bayesopt_vertical", False):
            out["proposals_vertical"] = acq.bayesopt_vert(write=write)
        if getattr(s, "bayesopt_nonvertical", False):
            out["proposals_nonvertical"] = acq.bayesopt_nonvert(write=write)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: python -m geobo_amd.run_geobo settings.yaml")
    run(sys.argv[1])
