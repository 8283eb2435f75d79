from torchain_amd.functions import ChainResults, _ChainLoss, best_path, chain_loss, den_best_path, den_expected_accuracy, den_expected_accuracy_dense, num_posteriors, to2d  # noqa: F401
