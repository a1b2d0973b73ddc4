"""Dataset fingerprint and experiment planners of nnunet/experiment_planning (DatasetAnalyzer.py, common_utils.py, the 3-D / 2-D planners
and the fork's custom_experiment_planner.py), with the reference's key names, file names, data identifiers and arithmetic, so that the
pickles written here are the ones the reference writes.

The planners are host arithmetic on a handful of numbers and import neither torch nor the library.  The fingerprint's one piece of
volume work -- the foreground samples `modality[seg > 0][::10]` of every cropped case -- runs on the device (ops.select_values: ranks
0, 10, 20, ... among the voxels with seg > 0); the statistics are then numpy's own calls on those float32 samples in the reference's
order, i.e. the reference's bits.  Not built: _load_seg_analyze_classes (analyze_dataset never calls it), -overwrite_plans, the
planners under alternative_experiment_planning/, the unlabeled planner.
"""
import os
import pickle
import shutil
from collections import OrderedDict
from copy import deepcopy

import numpy as np

from .folder_io import join, load_json, subfiles
from .safe_pickle import load_plain_pickle

default_data_identifier = "nnUNetData_plans_v2.1"      # nnunet/paths.py
default_num_threads = 8                                # nnunet/configuration.py


def save_pickle(obj, file):
    with open(file, "wb") as f:
        pickle.dump(obj, f)


def get_case_identifier_from_npz(case):
    return os.path.basename(case)[:-4]


def _task_folder_name(preprocessed_output_folder):
    """The fork's planners key two task-specific choices on digits anywhere in their output PATH ('28' in plans_fname, '027' in
    preprocessed_output_folder).  Here only the task folder's own name (`Task027_...`) is searched: the same answer under the reference's
    layout, and a parent folder that happens to hold those digits (a temporary folder, a date) changes nothing."""
    return os.path.basename(os.path.normpath(preprocessed_output_folder))


# ------------------------------------------------------------------------------------------------ generic_UNet.py constants
class Generic_UNet(object):
    """The planning constants and the memory estimate of network_architecture/generic_UNet.py:168-182, :411-449 (the network itself is
    cineflow.trainer's)."""
    DEFAULT_BATCH_SIZE_3D = 2
    BASE_NUM_FEATURES_3D = 30
    DEFAULT_BATCH_SIZE_2D = 50
    BASE_NUM_FEATURES_2D = 30
    use_this_for_batch_size_computation_2D = 19739648
    use_this_for_batch_size_computation_3D = 520000000

    @staticmethod
    def compute_approx_vram_consumption(patch_size, num_pool_per_axis, base_num_features, max_num_features, num_modalities, num_classes,
                                        pool_op_kernel_sizes, deep_supervision=False, conv_per_stage=2):
        """A number the memory use is roughly proportional to: feature-map voxels times channels over the encoder, the decoder and the
        transposed convolutions.  int64 throughout; the map size is divided with truncation, as an integer array divides in place."""
        size = np.array(patch_size)
        naxes = len(np.asarray(num_pool_per_axis))
        npool = len(pool_op_kernel_sizes)
        vox = np.prod(size, dtype=np.int64)
        total = np.int64((conv_per_stage * 2 + 1) * vox * base_num_features + num_modalities * vox + num_classes * vox)
        feat = base_num_features
        for p in range(npool):
            for a in range(naxes):
                size[a] = size[a] / pool_op_kernel_sizes[p][a]
            feat = min(feat * 2, max_num_features)
            blocks = (conv_per_stage * 2 + 1) if p < npool - 1 else conv_per_stage
            vox = np.prod(size, dtype=np.int64)
            total += blocks * vox * feat
            if deep_supervision and p < npool - 2:
                total += vox * num_classes
        return total


# ------------------------------------------------------------------------------------------------ common_utils.py
def get_shape_must_be_divisible_by(net_numpool_per_axis):
    return 2 ** np.array(net_numpool_per_axis)


def pad_shape(shape, must_be_divisible_by):
    """shape rounded up, axis by axis, to a multiple of must_be_divisible_by (a number or one per axis) -> int array"""
    if not isinstance(must_be_divisible_by, (tuple, list, np.ndarray)):
        must_be_divisible_by = [must_be_divisible_by] * len(shape)
    assert len(must_be_divisible_by) == len(shape)
    out = []
    for s, d in zip(shape, must_be_divisible_by):
        out.append(s if s % d == 0 else s + d - s % d)
    return np.array(out).astype(int)


def get_network_numpool(patch_size, maxpool_cap=999, min_feature_map_size=4):
    n = np.floor([np.log(i / min_feature_map_size) / np.log(2) for i in patch_size]).astype(int)
    return [min(i, maxpool_cap) for i in n]


def get_pool_and_conv_props_poolLateV2(patch_size, min_feature_map_size, max_numpool, spacing):
    """common_utils.py:50-86: every axis pools as often as its size allows, the axes with fewer poolings join late; a kernel is 3 along
    an axis once its spacing is within a factor 2 of the coarsest INITIAL spacing."""
    reach = max(deepcopy(spacing))
    dim = len(patch_size)
    num_pool_per_axis = get_network_numpool(patch_size, max_numpool, min_feature_map_size)
    net_numpool = max(num_pool_per_axis)
    pools, convs = [], []
    current = spacing
    for p in range(net_numpool):
        reached = [current[i] / reach > 0.5 for i in range(dim)]
        pool = [2 if num_pool_per_axis[i] + p >= net_numpool else 1 for i in range(dim)]
        convs.append([3] * dim if all(reached) else [1 if reached[i] else 3 for i in range(dim)])
        pools.append(pool)
        current = [i * j for i, j in zip(current, pool)]
    convs.append([3] * dim)
    divisible = get_shape_must_be_divisible_by(num_pool_per_axis)
    return num_pool_per_axis, pools, convs, pad_shape(patch_size, divisible), divisible


def get_pool_and_conv_props(spacing, patch_size, min_feature_map_size, max_numpool):
    """common_utils.py:89-154: pool the axes whose spacing is within a factor 2 of the finest one while their size allows it; the
    kernel is 3 along the largest group of axes whose spacings are within a factor 2 of each other."""
    dim = len(spacing)
    current_spacing = deepcopy(list(spacing))
    current_size = deepcopy(list(patch_size))
    pools, convs = [], []
    num_pool_per_axis = [0] * dim
    while True:
        finest = min(current_spacing)
        can_pool = [i for i in range(dim) if current_spacing[i] / finest < 2]
        group = []
        for a in range(dim):
            mine = current_spacing[a]
            partners = [i for i in range(dim) if current_spacing[i] / mine < 2 and mine / current_spacing[i] < 2]
            if len(partners) > len(group):
                group = partners
        conv = [3 if i in group else 1 for i in range(dim)]
        can_pool = [i for i in can_pool if current_size[i] >= 2 * min_feature_map_size]
        can_pool = [i for i in can_pool if num_pool_per_axis[i] < max_numpool]
        if len(can_pool) == 0:
            break
        pool = [1] * dim
        for v in can_pool:
            pool[v] = 2
            num_pool_per_axis[v] += 1
            current_spacing[v] *= 2
            current_size[v] = np.ceil(current_size[v] / 2)
        pools.append(pool)
        convs.append(conv)
    divisible = get_shape_must_be_divisible_by(num_pool_per_axis)
    convs.append([3] * dim)
    return num_pool_per_axis, pools, convs, pad_shape(patch_size, divisible), divisible


# ------------------------------------------------------------------------------------------------ DatasetAnalyzer.py
class DatasetAnalyzer(object):
    """DatasetAnalyzer.py:27-256 as nnUNet_plan_and_preprocess.py drives it.  num_processes: reader threads (at most 16)."""

    def __init__(self, folder_with_cropped_data, overwrite=True, num_processes=default_num_threads):
        self.num_processes = max(1, min(16, int(num_processes)))
        self.overwrite = overwrite
        self.folder_with_cropped_data = folder_with_cropped_data
        self.sizes = self.spacings = None
        self.patient_identifiers = [get_case_identifier_from_npz(i) for i in subfiles(folder_with_cropped_data, suffix=".npz")]
        assert os.path.isfile(join(folder_with_cropped_data, "dataset.json")), "dataset.json needs to be in folder_with_cropped_data"
        self.props_per_case_file = join(folder_with_cropped_data, "props_per_case.pkl")
        self.intensityproperties_file = join(folder_with_cropped_data, "intensityproperties.pkl")

    def load_properties_of_cropped(self, case_identifier):
        return load_plain_pickle(join(self.folder_with_cropped_data, "%s.pkl" % case_identifier))

    def _load_cropped(self, case_identifier):
        return np.load(join(self.folder_with_cropped_data, case_identifier) + ".npz")["data"]

    def _cases_on_device(self):
        """(identifier, device tensor [C + 1, X, Y, Z]) of every cropped case in order, the .npz files read ahead by a thread pool and each
        case uploaded once"""
        import torch
        from .folder_io import read_ahead
        dev = torch.device("cuda", torch.cuda.current_device())
        for group, loaded in read_ahead([[p] for p in self.patient_identifiers], self._load_cropped, depth=self.num_processes):
            yield group[0], torch.from_numpy(np.ascontiguousarray(loaded[0], dtype=np.float32)).to(dev)

    def get_classes(self):
        return load_json(join(self.folder_with_cropped_data, "dataset.json"))["labels"]

    def analyse_segmentations(self):
        """props_per_case.pkl: {case: {'has_classes': np.unique(seg)}} -- sorted unique values of the float32 label channel"""
        class_dct = self.get_classes()
        if self.overwrite or not os.path.isfile(self.props_per_case_file):
            import torch
            props_per_patient = OrderedDict()
            for p, t in self._cases_on_device():
                props_per_patient[p] = {"has_classes": torch.unique(t[-1]).cpu().numpy()}
            save_pickle(props_per_patient, self.props_per_case_file)
        else:
            props_per_patient = load_plain_pickle(self.props_per_case_file)
        return class_dct, props_per_patient

    def get_sizes_and_spacings_after_cropping(self):
        sizes, spacings = [], []
        for c in self.patient_identifiers:
            properties = self.load_properties_of_cropped(c)
            sizes.append(properties["size_after_cropping"])
            spacings.append(properties["original_spacing"])
        return sizes, spacings

    def get_modalities(self):
        modalities = load_json(join(self.folder_with_cropped_data, "dataset.json"))["modality"]
        return {int(k): modalities[k] for k in modalities.keys()}

    def get_size_reduction_by_cropping(self):
        size_reduction = OrderedDict()
        for p in self.patient_identifiers:
            props = self.load_properties_of_cropped(p)
            size_reduction[p] = np.prod(props["size_after_cropping"]) / np.prod(props["original_size_of_raw_data"])
        return size_reduction

    @staticmethod
    def _compute_stats(voxels):
        """DatasetAnalyzer.py:168-179: numpy's own calls on the list of float32 samples"""
        if len(voxels) == 0:
            return np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan
        return (np.median(voxels), np.mean(voxels), np.std(voxels), np.min(voxels), np.max(voxels), np.percentile(voxels, 99.5),
                np.percentile(voxels, 00.5))

    def _foreground_samples(self, num_modalities):
        """per modality, per case: list(modality[seg > 0][::10]) -- one count pass per case serves every modality"""
        from . import ops
        out = [[] for _ in range(num_modalities)]
        for _, t in self._cases_on_device():
            seg = t[-1].contiguous()
            index = ops.RankIndex(seg)
            ranks = np.arange(0, int(index.totals[0]), 10, dtype=np.int64)
            for m in range(num_modalities):
                out[m].append(list(ops.select_values(t[m].contiguous(), seg, ranks, index).cpu().numpy()))
        return out

    def collect_intensity_properties(self, num_modalities):
        if self.overwrite or not os.path.isfile(self.intensityproperties_file):
            names = ("median", "mean", "sd", "mn", "mx", "percentile_99_5", "percentile_00_5")
            samples = self._foreground_samples(num_modalities)
            results = OrderedDict()
            for mod_id in range(num_modalities):
                results[mod_id] = OrderedDict()
                v = samples[mod_id]
                w = []
                for iv in v:
                    w += iv
                whole = self._compute_stats(w)
                props_per_case = OrderedDict()
                for pat, iv in zip(self.patient_identifiers, v):
                    props_per_case[pat] = OrderedDict(zip(names, self._compute_stats(iv)))
                results[mod_id]["local_props"] = props_per_case
                for k, s in zip(names, whole):
                    results[mod_id][k] = s
            save_pickle(results, self.intensityproperties_file)
        else:
            results = load_plain_pickle(self.intensityproperties_file)
        return results

    def analyze_dataset(self, collect_intensityproperties=True):
        sizes, spacings = self.get_sizes_and_spacings_after_cropping()
        all_classes = [int(i) for i in self.get_classes().keys() if int(i) > 0]
        modalities = self.get_modalities()
        intensityproperties = self.collect_intensity_properties(len(modalities)) if collect_intensityproperties else None
        dataset_properties = dict()
        dataset_properties["all_sizes"] = sizes
        dataset_properties["all_spacings"] = spacings
        dataset_properties["all_classes"] = all_classes
        dataset_properties["modalities"] = modalities
        dataset_properties["intensityproperties"] = intensityproperties
        dataset_properties["size_reductions"] = self.get_size_reduction_by_cropping()
        save_pickle(dataset_properties, join(self.folder_with_cropped_data, "dataset_properties.pkl"))
        return dataset_properties


# ------------------------------------------------------------------------------------------------ planners
class ExperimentPlanner(object):
    """experiment_planner_baseline_3DUNet.py: pool-late 3-D U-Net, median target spacing, 3d_lowres stage when a patch sees less than a
    quarter of the median patient."""

    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        self.folder_with_cropped_data = folder_with_cropped_data
        self.preprocessed_output_folder = preprocessed_output_folder
        self.list_of_cropped_npz_files = subfiles(folder_with_cropped_data, suffix=".npz")
        self.preprocessor_name = "GenericPreprocessor"
        assert os.path.isfile(join(folder_with_cropped_data, "dataset_properties.pkl")), "folder_with_cropped_data must contain dataset_properties.pkl"
        self.dataset_properties = load_plain_pickle(join(folder_with_cropped_data, "dataset_properties.pkl"))
        self.plans_per_stage = OrderedDict()
        self.plans = OrderedDict()
        self.plans_fname = join(preprocessed_output_folder, "nnUNetPlans" + "fixed_plans_3D.pkl")
        self.data_identifier = default_data_identifier
        self.transpose_forward = [0, 1, 2]
        self.transpose_backward = [0, 1, 2]
        self.unet_base_num_features = Generic_UNet.BASE_NUM_FEATURES_3D
        self.unet_max_num_filters = 320
        self.unet_max_numpool = 999
        self.unet_min_batch_size = 2
        self.unet_featuremap_min_edge_length = 4
        self.target_spacing_percentile = 50
        self.anisotropy_threshold = 3
        self.how_much_of_a_patient_must_the_network_see_at_stage0 = 4
        self.batch_size_covers_max_percent_of_dataset = 0.05
        self.conv_per_stage = 2

    # -- pieces the subclasses choose
    def _pool_props(self, spacing, patch_size):
        return get_pool_and_conv_props_poolLateV2(patch_size, self.unet_featuremap_min_edge_length, self.unet_max_numpool, spacing)

    def _budget_3d(self):
        return Generic_UNet.use_this_for_batch_size_computation_3D

    def _vram(self, shape, numpool, features, num_modalities, num_classes, pools):
        return Generic_UNet.compute_approx_vram_consumption(shape, numpool, features, self.unet_max_num_filters, num_modalities, num_classes, pools,
                                                            conv_per_stage=self.conv_per_stage)

    def _shrink_to_budget(self, spacing, shape, median_shape, ref, first_features, num_modalities, num_classes):
        """the `while here > ref` loop every planner shares: take one divisibility step off the axis that is largest relative to the
        median shape until the estimate fits -> (numpool, pools, convs, shape, here)"""
        numpool, pools, convs, shape, divisible = self._pool_props(spacing, shape)
        here = self._vram(shape, numpool, first_features, num_modalities, num_classes, pools)
        while here > ref:
            axis = np.argsort(shape / median_shape)[-1]
            tmp = deepcopy(shape)
            tmp[axis] -= divisible[axis]
            divisible_new = self._pool_props(spacing, tmp)[4]
            shape[axis] -= divisible_new[axis]
            numpool, pools, convs, shape, divisible = self._pool_props(spacing, shape)
            here = self._vram(shape, numpool, self.unet_base_num_features, num_modalities, num_classes, pools)
        return numpool, pools, convs, shape, here

    def get_target_spacing(self):
        return np.percentile(np.vstack(self.dataset_properties["all_spacings"]), self.target_spacing_percentile, 0)

    def save_my_plans(self):
        save_pickle(self.plans, self.plans_fname)

    def load_my_plans(self):
        self.plans = load_plain_pickle(self.plans_fname)
        self.plans_per_stage = self.plans["plans_per_stage"]
        self.dataset_properties = self.plans["dataset_properties"]
        self.transpose_forward = self.plans["transpose_forward"]
        self.transpose_backward = self.plans["transpose_backward"]

    def get_properties_for_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        new_median_shape = np.round(original_spacing / current_spacing * original_shape).astype(int)
        dataset_num_voxels = np.prod(new_median_shape) * num_cases
        # an isotropic 512 mm patch in voxels, clipped to the median shape
        patch = 1 / np.array(current_spacing)
        patch /= patch.mean()
        patch *= 1 / min(patch) * 512
        patch = np.round(patch).astype(int)
        patch = [min(i, j) for i, j in zip(patch, new_median_shape)]
        ref = self._budget_3d()
        numpool, pools, convs, patch, here = self._shrink_to_budget(current_spacing, patch, new_median_shape, ref, self.unet_base_num_features,
                                                                    num_modalities, num_classes)
        batch_size = int(np.floor(max(ref / here, 1) * Generic_UNet.DEFAULT_BATCH_SIZE_3D))
        max_batch_size = np.round(self.batch_size_covers_max_percent_of_dataset * dataset_num_voxels / np.prod(patch, dtype=np.int64)).astype(int)
        max_batch_size = max(max_batch_size, self.unet_min_batch_size)
        batch_size = max(1, min(batch_size, max_batch_size))
        return {
            "batch_size": batch_size,
            "num_pool_per_axis": numpool,
            "patch_size": patch,
            "median_patient_size_in_voxels": new_median_shape,
            "current_spacing": current_spacing,
            "original_spacing": original_spacing,
            "do_dummy_2D_data_aug": (max(patch) / patch[0]) > self.anisotropy_threshold,
            "pool_op_kernel_sizes": pools,
            "conv_kernel_sizes": convs,
        }

    def _transposes(self, target_spacing):
        first = np.argmax(target_spacing)
        self.transpose_forward = [first] + [i for i in range(3) if i != first]
        self.transpose_backward = [np.argwhere(np.array(self.transpose_forward) == i)[0][0] for i in range(3)]

    def _assemble(self, num_modalities, modalities, spacings, sizes, all_classes, use_mask):
        return {"num_stages": len(list(self.plans_per_stage.keys())), "num_modalities": num_modalities, "modalities": modalities,
                "normalization_schemes": self.determine_normalization_scheme(), "dataset_properties": self.dataset_properties,
                "list_of_npz_files": self.list_of_cropped_npz_files, "original_spacings": spacings, "original_sizes": sizes,
                "preprocessed_data_folder": self.preprocessed_output_folder, "num_classes": len(all_classes), "all_classes": all_classes,
                "base_num_features": self.unet_base_num_features, "use_mask_for_norm": use_mask, "keep_only_largest_region": None,
                "min_region_size_per_class": None, "min_size_per_class": None, "transpose_forward": self.transpose_forward,
                "transpose_backward": self.transpose_backward, "data_identifier": self.data_identifier, "plans_per_stage": self.plans_per_stage,
                "preprocessor_name": self.preprocessor_name}

    def plan_experiment(self):
        use_mask = self.determine_whether_to_use_mask_for_norm()
        spacings, sizes = self.dataset_properties["all_spacings"], self.dataset_properties["all_sizes"]
        all_classes, modalities = self.dataset_properties["all_classes"], self.dataset_properties["modalities"]
        num_modalities = len(list(modalities.keys()))
        target_spacing = self.get_target_spacing()
        new_shapes = [np.array(i) / target_spacing * np.array(j) for i, j in zip(spacings, sizes)]
        self._transposes(target_spacing)
        median_shape = np.median(np.vstack(new_shapes), 0)
        target_t = np.array(target_spacing)[self.transpose_forward]
        median_t = np.array(median_shape)[self.transpose_forward]
        num_cases = len(self.list_of_cropped_npz_files)
        stages = [self.get_properties_for_stage(target_t, target_t, median_t, num_cases, num_modalities, len(all_classes) + 1)]
        seen = np.prod(stages[-1]["patch_size"], dtype=np.int64)
        quarter = self.how_much_of_a_patient_must_the_network_see_at_stage0
        if not np.prod(median_shape) / seen < quarter:
            # 3d_lowres: coarsen (the finer axes first, until no axis is more than twice as fine as the coarsest) in steps of 1 % until the
            # median patient holds at most `quarter` patches of the stage planned at that spacing
            lowres = deepcopy(target_spacing)
            num_voxels = np.prod(median_shape, dtype=np.float64)
            while num_voxels > quarter * seen:
                coarsest = max(lowres)
                if np.any((coarsest / lowres) > 2):
                    lowres[(coarsest / lowres) > 2] *= 1.01
                else:
                    lowres *= 1.01
                num_voxels = np.prod(target_spacing / lowres * median_shape, dtype=np.float64)
                new = self.get_properties_for_stage(np.array(lowres)[self.transpose_forward], target_t, median_t, num_cases, num_modalities,
                                                    len(all_classes) + 1)
                seen = np.prod(new["patch_size"], dtype=np.int64)
            if 2 * np.prod(new["median_patient_size_in_voxels"], dtype=np.int64) < np.prod(stages[0]["median_patient_size_in_voxels"], dtype=np.int64):
                stages.append(new)
        stages = stages[::-1]
        self.plans_per_stage = {i: stages[i] for i in range(len(stages))}
        self.plans = self._assemble(num_modalities, modalities, spacings, sizes, all_classes, use_mask)
        self.plans["conv_per_stage"] = self.conv_per_stage
        self.save_my_plans()

    def determine_normalization_scheme(self):
        schemes = OrderedDict()
        modalities = self.dataset_properties["modalities"]
        for i in range(len(list(modalities.keys()))):
            if modalities[i] == "CT" or modalities[i] == "ct":
                schemes[i] = "CT"
            elif modalities[i] == "noNorm":
                schemes[i] = "noNorm"
            else:
                schemes[i] = "nonCT"
        return schemes

    def save_properties_of_cropped(self, case_identifier, properties):
        save_pickle(properties, join(self.folder_with_cropped_data, "%s.pkl" % case_identifier))

    def load_properties_of_cropped(self, case_identifier):
        return load_plain_pickle(join(self.folder_with_cropped_data, "%s.pkl" % case_identifier))

    def determine_whether_to_use_mask_for_norm(self):
        """the non-zero mask normalises a modality when cropping to it shrank the median case below 3/4 (never for CT); the decision is
        written back into every cropped case's .pkl"""
        modalities = self.dataset_properties["modalities"]
        use = OrderedDict()
        for i in range(len(list(modalities.keys()))):
            if "CT" in modalities[i]:
                use[i] = False
            else:
                reductions = [self.dataset_properties["size_reductions"][k] for k in self.dataset_properties["size_reductions"].keys()]
                use[i] = bool(np.median(reductions) < 3 / 4.)
        for c in self.list_of_cropped_npz_files:
            case_identifier = get_case_identifier_from_npz(c)
            properties = self.load_properties_of_cropped(case_identifier)
            properties["use_nonzero_mask_for_norm"] = use
            self.save_properties_of_cropped(case_identifier, properties)
        return use

    def _preprocessor(self):
        from . import preprocessing
        cls = getattr(preprocessing, self.preprocessor_name)
        return cls(self.plans["normalization_schemes"], self.plans["use_mask_for_norm"], self.transpose_forward,
                   self.plans["dataset_properties"]["intensityproperties"])

    def run_preprocessing(self, num_threads, keep_spacing=False, preprocessor=None):
        """preprocessor: an instance made by _preprocessor() that the caller wants to keep (its `seconds` hold the time split)"""
        gt = join(self.preprocessed_output_folder, "gt_segmentations")
        if os.path.isdir(gt):
            shutil.rmtree(gt)
        shutil.copytree(join(self.folder_with_cropped_data, "gt_segmentations"), gt)
        target_spacings = [i["current_spacing"] for i in self.plans_per_stage.values()]
        if isinstance(num_threads, (list, tuple)):
            num_threads = num_threads[-1]
        (preprocessor or self._preprocessor()).run(target_spacings, self.folder_with_cropped_data, self.preprocessed_output_folder, self.plans["data_identifier"],
                                 num_threads, keep_spacing=keep_spacing)


class ExperimentPlanner3D_v21(ExperimentPlanner):
    """experiment_planner_baseline_3DUNet_v21.py: pooling by spacing, 32 base features, and a finer target spacing along a
    low-resolution axis of anisotropic datasets."""

    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        super(ExperimentPlanner3D_v21, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = "nnUNetData_plans_v2.1"
        self.plans_fname = join(self.preprocessed_output_folder, "nnUNetPlansv2.1_plans_3D.pkl")
        self.unet_base_num_features = 32

    def _pool_props(self, spacing, patch_size):
        return get_pool_and_conv_props(spacing, patch_size, self.unet_featuremap_min_edge_length, self.unet_max_numpool)

    def _budget_3d(self):
        return Generic_UNet.use_this_for_batch_size_computation_3D * self.unet_base_num_features / Generic_UNet.BASE_NUM_FEATURES_3D

    def get_target_spacing(self):
        spacings, sizes = self.dataset_properties["all_spacings"], self.dataset_properties["all_sizes"]
        target = np.percentile(np.vstack(spacings), self.target_spacing_percentile, 0)
        target_size = np.percentile(np.vstack(sizes), self.target_spacing_percentile, 0)
        worst = np.argmax(target)
        others = [i for i in range(len(target)) if i != worst]
        other_spacings = [target[i] for i in others]
        other_sizes = [target_size[i] for i in others]
        aniso_spacing = target[worst] > (self.anisotropy_threshold * max(other_spacings))
        aniso_voxels = target_size[worst] * self.anisotropy_threshold < min(other_sizes)
        if aniso_spacing and aniso_voxels:
            # the 10th percentile of that axis' spacings, but never finer than the other axes
            finer = np.percentile(np.vstack(spacings)[:, worst], 10)
            if finer < max(other_spacings):
                finer = max(max(other_spacings), finer) + 1e-5
            target[worst] = finer
        return target


class ExperimentPlanner2D(ExperimentPlanner):
    """experiment_planner_baseline_2DUNet.py: one stage, whole median slices as patches."""

    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        super(ExperimentPlanner2D, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = default_data_identifier + "_2D"
        self.plans_fname = join(self.preprocessed_output_folder, "nnUNetPlans" + "_plans_2D.pkl")
        self.unet_base_num_features = 30
        self.unet_max_num_filters = 512
        self.unet_max_numpool = 999
        self.preprocessor_name = "PreprocessorFor2D"

    def _pool_props(self, spacing, patch_size):
        return get_pool_and_conv_props(spacing, patch_size, self.unet_featuremap_min_edge_length, self.unet_max_numpool)

    def _stage_dict(self, batch_size, numpool, patch, median, current_spacing, original_spacing, pools, convs):
        return {"batch_size": batch_size, "num_pool_per_axis": numpool, "patch_size": patch, "median_patient_size_in_voxels": median,
                "current_spacing": current_spacing, "original_spacing": original_spacing, "pool_op_kernel_sizes": pools,
                "conv_kernel_sizes": convs, "do_dummy_2D_data_aug": False}

    def _cap_batch(self, batch_size, dataset_num_voxels, patch):
        cap = np.round(self.batch_size_covers_max_percent_of_dataset * dataset_num_voxels / np.prod(patch, dtype=np.int64)).astype(int)
        return max(1, min(batch_size, cap))

    def get_properties_for_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        new_median_shape = np.round(original_spacing / current_spacing * original_shape).astype(int)
        dataset_num_voxels = np.prod(new_median_shape, dtype=np.int64) * num_cases
        numpool, pools, convs, patch, _ = self._pool_props(current_spacing[1:], new_median_shape[1:])
        estimate = self._vram(patch, numpool, self.unet_base_num_features, num_modalities, num_classes, pools)
        batch_size = int(np.floor(Generic_UNet.use_this_for_batch_size_computation_2D / estimate * Generic_UNet.DEFAULT_BATCH_SIZE_2D))
        if batch_size < self.unet_min_batch_size:
            raise RuntimeError("This framework is not made to process patches this large. We will add patch-based 2D networks later. "
                               "Sorry for the inconvenience")
        batch_size = self._cap_batch(batch_size, dataset_num_voxels, patch)
        return self._stage_dict(batch_size, numpool, patch, new_median_shape, current_spacing, original_spacing, pools, convs)

    def _budgeted_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        """the v2.1 form both later 2-D planners share: patch shrunk until the estimate fits a batch of two"""
        new_median_shape = np.round(original_spacing / current_spacing * original_shape).astype(int)
        dataset_num_voxels = np.prod(new_median_shape, dtype=np.int64) * num_cases
        ref = Generic_UNet.use_this_for_batch_size_computation_2D * Generic_UNet.DEFAULT_BATCH_SIZE_2D / 2
        # the first estimate pretends 30 features (the configuration of the baseline planner); inside the loop the planner's own count
        numpool, pools, convs, patch, here = self._shrink_to_budget(current_spacing[1:], new_median_shape[1:], new_median_shape[1:], ref, 30,
                                                                    num_modalities, num_classes)
        batch_size = int(np.floor(ref / here) * 2)
        if batch_size < self.unet_min_batch_size:
            raise RuntimeError("This should not happen")
        batch_size = self._cap_batch(batch_size, dataset_num_voxels, patch)
        return self._stage_dict(batch_size, numpool, patch, new_median_shape, current_spacing, original_spacing, pools, convs)

    def plan_experiment(self):
        use_mask = self.determine_whether_to_use_mask_for_norm()
        spacings, sizes = self.dataset_properties["all_spacings"], self.dataset_properties["all_sizes"]
        all_classes, modalities = self.dataset_properties["all_classes"], self.dataset_properties["modalities"]
        num_modalities = len(list(modalities.keys()))
        target_spacing = self.get_target_spacing()
        new_shapes = np.array([np.array(i) / target_spacing * np.array(j) for i, j in zip(spacings, sizes)])
        if "28" in _task_folder_name(self.preprocessed_output_folder):       # (the fork's task 28: slices along the finest axis)
            first = np.argmin(target_spacing)
            self.transpose_forward = [first] + [i for i in range(3) if i != first]
            self.transpose_backward = [np.argwhere(np.array(self.transpose_forward) == i)[0][0] for i in range(3)]
        else:
            self._transposes(target_spacing)
        median_shape = np.median(np.vstack(new_shapes), 0)
        target_t = np.array(target_spacing)[self.transpose_forward]
        median_t = np.array(median_shape)[self.transpose_forward]
        stage = self.get_properties_for_stage(target_t, target_t, median_t, num_cases=len(self.list_of_cropped_npz_files),
                                              num_modalities=num_modalities, num_classes=len(all_classes) + 1)
        self.plans_per_stage = {0: stage}
        self.plans = self._assemble(num_modalities, modalities, spacings, sizes, all_classes, use_mask)
        self.save_my_plans()


class ExperimentPlanner2D_v21(ExperimentPlanner2D):
    """experiment_planner_baseline_2DUNet_v21.py"""

    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        super(ExperimentPlanner2D_v21, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = "nnUNetData_plans_v2.1_2D"
        self.plans_fname = join(self.preprocessed_output_folder, "nnUNetPlansv2.1_plans_2D.pkl")
        self.unet_base_num_features = 32

    def get_properties_for_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        return self._budgeted_stage(current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes)


class CustomExperimentPlanner(ExperimentPlanner2D):
    """custom_experiment_planner.py:23-108: batch size, pooling depth and patch size come from the model's YAML (batch_size,
    in_encoder_dims), patch 224 for task 027 and 288 otherwise.  config: the YAML file (the reference reads adversarial_acdc.yaml from
    the working directory) or the mapping it holds."""

    def __init__(self, folder_with_cropped_data, preprocessed_output_folder, config=None):
        super(CustomExperimentPlanner, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = "custom_experiment_planner"
        self.plans_fname = join(self.preprocessed_output_folder, "custom_experiment_planner_plans_2D.pkl")
        self.unet_base_num_features = 32
        if config is None:
            raise ValueError("CustomExperimentPlanner needs the model's YAML (--planner_config): it holds batch_size and in_encoder_dims")
        if not isinstance(config, dict):
            import yaml
            with open(config) as f:
                config = yaml.safe_load(f)
        self.config = config
        self.patch_size = 224 if "027" in _task_folder_name(self.preprocessed_output_folder) else 288

    def get_properties_for_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        plan = self._budgeted_stage(current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes)
        depth = len(self.config["in_encoder_dims"])
        plan["batch_size"] = self.config["batch_size"]
        plan["num_pool_per_axis"] = [depth, depth]
        plan["patch_size"] = np.array([self.patch_size, self.patch_size])
        plan["pool_op_kernel_sizes"] = [[2, 2], [2, 2], [2, 2]]
        return plan


PLANNERS = {c.__name__: c for c in (ExperimentPlanner, ExperimentPlanner3D_v21, ExperimentPlanner2D, ExperimentPlanner2D_v21, CustomExperimentPlanner)}


def find_planner(name):
    """the planner class of that name; None for None / 'None'.  A name this build does not have raises NotImplementedError."""
    if name is None or name == "None":
        return None
    if name not in PLANNERS:
        raise NotImplementedError("planner %r is not built (built: %s)" % (name, ", ".join(sorted(PLANNERS))))
    return PLANNERS[name]
