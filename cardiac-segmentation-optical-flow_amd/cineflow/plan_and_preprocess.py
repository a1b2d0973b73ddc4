"""nnUNet_plan_and_preprocess (nnunet/experiment_planning/nnUNet_plan_and_preprocess.py) on the device: a raw task folder becomes the
cropped cases, the dataset fingerprint, the plans files and the resampled, normalised stage folders with class locations.

    python -m cineflow.plan_and_preprocess --raw TASK_FOLDER --cropped DIR --preprocessed DIR [-pl3d NAME|None] [-pl2d NAME|None]
                                           [--planner_config YAML] [-no_pp] [-tf N]
    python -m cineflow.plan_and_preprocess -t ID ...      # folders from nnUNet_raw_data_base / nnUNet_preprocessed, the reference's layout

Not served: unlabeled cases, --verify_dataset_integrity, -overwrite_plans, the planners of alternative_experiment_planning/ (INTEGRATION.md).
"""
import argparse
import ntpath
import os
import shutil
import sys
import time

from . import experiment_planning as EP
from .folder_io import join, load_json


def create_lists_from_splitted_dataset(base_folder_splitted):
    """experiment_planning/utils.py:114-147 -> (patients -> cases -> [image file per modality ..., label file], {index: modality},
    patients -> cases -> the dataset.json training entry).  A patient is the file-name prefix before the first `_`; patients and their
    cases keep dataset.json's order."""
    d = load_json(join(base_folder_splitted, "dataset.json"))
    num_modalities = len(d["modality"].keys())
    by_patient = {}
    for tr in d["training"]:
        name = ntpath.basename(tr["image"]).split("_")[0]
        case = [join(base_folder_splitted, "imagesTr", tr["image"].split("/")[-1][:-7] + "_%04.0d.nii.gz" % m) for m in range(num_modalities)]
        case.append(join(base_folder_splitted, "labelsTr", tr["label"].split("/")[-1]))
        cases, infos = by_patient.setdefault(name, ([], []))
        cases.append(case)
        infos.append(tr)
    lists = [v[0] for v in by_patient.values()]
    info_list = [v[1] for v in by_patient.values()]
    return lists, {int(i): d["modality"][str(i)] for i in d["modality"].keys()}, info_list


def crop(raw_task_folder, cropped_out_dir, override=False, num_threads=EP.default_num_threads, compress="zlib"):
    """experiment_planning/utils.py:207-222 -> the ImageCropper that ran (its `seconds` say where the time went)"""
    from .preprocessing import ImageCropper
    if override and os.path.isdir(cropped_out_dir):
        shutil.rmtree(cropped_out_dir)
    os.makedirs(cropped_out_dir, exist_ok=True)
    lists, _, info_list = create_lists_from_splitted_dataset(raw_task_folder)
    imgcrop = ImageCropper(num_threads, cropped_out_dir, compress)
    imgcrop.run_cropping(lists, overwrite_existing=override, info_list=info_list)
    shutil.copy(join(raw_task_folder, "dataset.json"), cropped_out_dir)
    return imgcrop


def convert_id_to_task_name(task_id, folders):
    """the one `Task%03d_*` folder name under the given folders (nnunet/utilities/task_name_id_conversion.py)"""
    prefix = "Task%03.0d" % task_id
    names = sorted({n for f in folders if f and os.path.isdir(f) for n in os.listdir(f) if n.startswith(prefix) and os.path.isdir(join(f, n))})
    if len(names) != 1:
        raise RuntimeError("%d folders start with %s under %s" % (len(names), prefix, [f for f in folders if f]))
    return names[0]


def plan_and_preprocess(raw, cropped, preprocessed, planner3d="ExperimentPlanner3D_v21", planner2d="ExperimentPlanner2D_v21", planner_config=None,
                        no_pp=False, tf=8, report=None, compress="zlib"):
    """One task.  report: a dict that receives the seconds per step (tools/plan_and_preprocess_bench.py).  compress="device": every .npz
    (cropped cases, stage folders) is deflated and checksummed on the device (cineflow.deflate); the arrays inside are the same."""
    from .deflate import check_compress
    check_compress(compress)
    tf = max(1, min(16, int(tf)))
    planners = [EP.find_planner(planner3d), EP.find_planner(planner2d)]           # an unknown name raises before any work
    report = {} if report is None else report
    t0 = time.perf_counter()
    report["crop"] = dict(crop(raw, cropped, False, tf, compress).seconds)
    report["crop"]["total"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    modalities = list(load_json(join(cropped, "dataset.json"))["modality"].values())
    collect = ("CT" in modalities) or ("ct" in modalities)
    analyzer = EP.DatasetAnalyzer(cropped, overwrite=False, num_processes=tf)
    analyzer.analyze_dataset(collect)
    analyzer.analyse_segmentations()          # props_per_case.pkl (the reference's script leaves this one to its callers)
    report["fingerprint"] = {"total": time.perf_counter() - t0}

    os.makedirs(preprocessed, exist_ok=True)
    shutil.copy(join(cropped, "dataset_properties.pkl"), preprocessed)
    shutil.copy(join(raw, "dataset.json"), preprocessed)
    for cls in planners:
        if cls is None:
            continue
        planner = cls(cropped, preprocessed, planner_config) if cls is EP.CustomExperimentPlanner else cls(cropped, preprocessed)
        planner.plan_experiment()
        if not no_pp:
            t0 = time.perf_counter()
            pre = planner._preprocessor()
            pre.compress = compress
            planner.run_preprocessing(tf, preprocessor=pre)
            report[planner.data_identifier] = dict(pre.seconds, total=time.perf_counter() - t0, stages=len(planner.plans_per_stage))
    return report


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cineflow.plan_and_preprocess", description=__doc__.split("\n\n")[0])
    ap.add_argument("-t", "--task_ids", nargs="+", default=None, help="task ids; the folders then follow the reference's layout under "
                    "$nnUNet_raw_data_base and $nnUNet_preprocessed")
    ap.add_argument("--raw", help="raw task folder (imagesTr, labelsTr, dataset.json)")
    ap.add_argument("--cropped", help="folder for the cropped cases and the fingerprint")
    ap.add_argument("--preprocessed", help="folder for the plans and the stage folders")
    ap.add_argument("-pl3d", "--planner3d", default="ExperimentPlanner3D_v21")
    ap.add_argument("-pl2d", "--planner2d", default="ExperimentPlanner2D_v21")
    ap.add_argument("--planner_config", default=None, help="the model's YAML for CustomExperimentPlanner")
    ap.add_argument("-no_pp", action="store_true", help="plan only: write the plans files and no stage folder")
    ap.add_argument("-tf", type=int, default=8, help="reader / writer threads (at most 16)")
    ap.add_argument("--compress", choices=("zlib", "device"), default="zlib", help="who deflates the .npz files: zlib on the writer threads "
                    "(default) or the device, which then hands back compressed bytes only; the arrays inside are identical")
    a = ap.parse_args(argv)
    if a.task_ids:
        base, pre = os.environ.get("nnUNet_raw_data_base"), os.environ.get("nnUNet_preprocessed")
        if not base or not pre:
            ap.error("-t needs the environment variables nnUNet_raw_data_base and nnUNet_preprocessed")
        raw_root, cropped_root = join(base, "nnUNet_raw_data"), join(base, "nnUNet_cropped_data")
        jobs = []
        for i in a.task_ids:
            name = convert_id_to_task_name(int(i), [raw_root])
            jobs.append((join(raw_root, name), join(cropped_root, name), join(pre, name)))
    else:
        if not (a.raw and a.cropped and a.preprocessed):
            ap.error("give --raw, --cropped and --preprocessed, or -t with the reference's environment variables")
        jobs = [(a.raw, a.cropped, a.preprocessed)]
    for raw, cropped, preprocessed in jobs:
        report = plan_and_preprocess(raw, cropped, preprocessed, a.planner3d, a.planner2d, a.planner_config, a.no_pp, a.tf, compress=a.compress)
        print("%s: %s" % (preprocessed, {k: round(v["total"], 3) for k, v in report.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
