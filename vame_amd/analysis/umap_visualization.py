"""UMAP plots of the latent vectors -- drop-in for vame/analysis/umap_visualization.py (`vame.visualization(config, label=None)`).

Same file selection and prompts (:53-74), the same input (results/<file>/<model>/<parameterization>-<n_cluster>/latent_vector_<file>.npy,
first num_points rows), the same output (community/umap_embedding_<file>.npy, reused when it exists: :78-84) and the same three
scatter plots (no label, 'motif', 'community': :20-44, 98-111).  The embedding comes from umap-learn when it is installed (the
reference's exact behaviour) or, with amd_gpu_umap: True in config.yaml, from the MI355X implementation (umap_hip.UMAPHIP).
"""
import os
from pathlib import Path

import numpy as np
import torch.distributed as dist

from ..model.evaluate import _pyplot
from ..util.auxiliary import read_config
from .pose_segmentation import _ask


def _umap_cls(cfg):
    """umap-learn's UMAP unless cfg['amd_gpu_umap'] is set; then UMAPHIP (vame_amd/analysis/umap_hip.py).  The GPU layout is never
    chosen silently: it is not bit-identical to umap-learn's."""
    if cfg.get('amd_gpu_umap', False):
        from .umap_hip import UMAPHIP
        return UMAPHIP
    try:
        import umap
    except ImportError as e:
        raise ImportError("visualization() needs umap-learn (as in the reference); to compute the UMAP embedding on the MI355X instead "
                          "set amd_gpu_umap: True in config.yaml") from e
    return umap.UMAP


def umap_vis(file, embed, num_points):
    plt = _pyplot()
    plt.figure(1)
    plt.scatter(embed[:num_points, 0], embed[:num_points, 1], s=2, alpha=.5)
    plt.gca().set_aspect('equal', 'datalim')
    plt.grid(False)


def umap_label_vis(file, embed, label, n_cluster, num_points):
    plt = _pyplot()
    plt.figure(1)
    plt.scatter(embed[:num_points, 0], embed[:num_points, 1], c=label[:num_points], cmap='Spectral', s=2, alpha=.7)
    plt.colorbar(boundaries=np.arange(n_cluster + 1) - 0.5).set_ticks(np.arange(n_cluster))
    plt.gca().set_aspect('equal', 'datalim')
    plt.grid(False)


def umap_vis_comm(file, embed, community_label, num_points):
    plt = _pyplot()
    num = np.unique(community_label).shape[0]
    plt.figure(1)
    plt.scatter(embed[:num_points, 0], embed[:num_points, 1], c=community_label[:num_points], cmap='Spectral', s=2, alpha=.7)
    plt.colorbar(boundaries=np.arange(num + 1) - 0.5).set_ticks(np.arange(num))
    plt.gca().set_aspect('equal', 'datalim')
    plt.grid(False)


def visualization(config, label=None):
    config_file = Path(config).resolve()
    cfg = read_config(config_file)
    model_name = cfg['model_name']
    n_cluster = cfg['n_cluster']
    param = cfg['parameterization']
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)

    def input(prompt):                               # noqa: A001  several ranks: ask on rank 0 only, every rank gets the answer
        return _ask(prompt, rank, world)

    files = []
    if cfg['all_data'] == 'No':
        all_flag = input("Do you want to write motif videos for your entire dataset? \n"
                         "If you only want to use a specific dataset type filename: \n"
                         "yes/no/filename ")
    else:
        all_flag = 'yes'
    if all_flag in ('yes', 'Yes'):
        files = list(cfg['video_sets'])
    elif all_flag in ('no', 'No'):
        for file in cfg['video_sets']:
            if input("Do you want to quantify " + file + "? yes/no: ") == 'yes':
                files.append(file)
    else:
        files.append(all_flag)

    for file in files:
        path_to_file = os.path.join(cfg['project_path'], "results", file, model_name, param + '-' + str(n_cluster))
        embed_path = os.path.join(path_to_file, "community", "umap_embedding_" + file + ".npy")
        if os.path.exists(embed_path):
            embed = np.load(embed_path)
            num_points = min(cfg['num_points'], embed.shape[0])
        else:
            os.makedirs(os.path.join(path_to_file, "community"), exist_ok=True)
            print("Compute embedding for file %s" % file)
            UMAP = _umap_cls(cfg)
            reducer = UMAP(n_components=2, min_dist=cfg['min_dist'], n_neighbors=cfg['n_neighbors'], random_state=cfg['random_state'])
            latent_vector = np.load(os.path.join(path_to_file, 'latent_vector_' + file + '.npy'))
            num_points = min(cfg['num_points'], latent_vector.shape[0])
            print("Embedding %d data points.." % num_points)
            embed = np.asarray(reducer.fit_transform(latent_vector[:num_points, :]), dtype=np.float32)
            if rank == 0:
                np.save(embed_path, embed)

        print("Visualizing %d data points.. " % num_points)
        if label is None:
            umap_vis(file, embed, num_points)
        if label == 'motif':
            motif_label = np.load(os.path.join(path_to_file, str(n_cluster) + '_km_label_' + file + '.npy'))
            umap_label_vis(file, embed, motif_label, n_cluster, num_points)
        if label == "community":
            comm_path = os.path.join(path_to_file, "community", "community_label_" + file + ".npy")
            if not os.path.exists(comm_path):
                raise FileNotFoundError(f"{comm_path} does not exist: label='community' needs the community labels that the reference's "
                                        "vame.community() writes, and community() is not part of vame_amd")
            umap_vis_comm(file, embed, np.load(comm_path), num_points)
