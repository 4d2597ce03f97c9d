"""Waveform input for the device front end (`frontend.FrontEnd`): 16-bit mono PCM .wav files through the standard library's `wave`
module, and Kaldi `wav.scp` tables of plain paths.  Anything else — other sample widths, several channels, another sample rate, a
piped command — is refused by name: there is no resampling and no decoding of other formats here."""
import wave

import numpy


def read_wav(path, sample_rate=16000.0):
    """-> 1-D int16 array of the samples.  `sample_rate`: the front end's (`FrontEnd.sample_rate`); None accepts any."""
    with wave.open(str(path), "rb") as f:
        if f.getsampwidth() != 2:
            raise ValueError("%s: sample width of %d bytes; only 16-bit PCM is read" % (path, f.getsampwidth()))
        if f.getnchannels() != 1:
            raise ValueError("%s: %d channels; only mono is read" % (path, f.getnchannels()))
        if sample_rate is not None and f.getframerate() != int(round(float(sample_rate))):
            raise ValueError("%s: sample rate %d Hz, the front end works at %d Hz (no sample-rate conversion is built)"
                             % (path, f.getframerate(), int(round(float(sample_rate)))))
        data = f.readframes(f.getnframes())
    return numpy.frombuffer(data, dtype="<i2").astype(numpy.int16)


def read_wav_scp(path):
    """Kaldi wav.scp, one `<id> <path>` per line -> list of (id, path).  A line whose entry is a command (ending in `|`) is refused."""
    entries = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split(None, 1)
            if len(parts) != 2:
                raise ValueError("%s:%d: expected `<id> <path>`, got %r" % (path, number, line))
            if parts[1].rstrip().endswith("|"):
                raise ValueError("%s:%d: utterance %s is a piped command (%r); piped wav.scp entries are not run, write the audio to "
                                 ".wav files first" % (path, number, parts[0], parts[1]))
            entries.append((parts[0], parts[1].strip()))
    return entries
