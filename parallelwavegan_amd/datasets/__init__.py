from .audio_mel_dataset import AudioMelDataset, MelDataset, find_files  # noqa: F401
